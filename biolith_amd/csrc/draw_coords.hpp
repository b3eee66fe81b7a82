// draw_coords.hpp -- where a handle's optional coordinates sit in a posterior draw, as every post-fit kernel is told (host and device).
// biolith_hip.hip fills it in one place (draw_coords) from the handle; the kernels' params structs embed it as `c`.
#pragma once

struct BlDrawCoords {
    int fp_mode;       // the handle's false-positive mode: 0 = no rate, BL_FP_CONSTANT (1), BL_FP_UNOCCUPIED (2)
    int o_fp;          // the rate's coordinate phi (logit of a probability; occu_cop: log of a rate); -1 = no rate
    int o_u, o_v, o_e; // random effects (external order: site occupancy / abundance [N], site detection [N], visit [N][T][J]); -1 = absent
};
