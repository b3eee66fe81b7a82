// pred_rng.hpp -- the generator of the post-fit kernels (bl_predict*, bl_site_posterior).
// One generator per (draw, period, site): xoshiro128++ keyed by splitmix64 of the flat index, so the
// sample does not depend on the launch geometry or on how the draws are chunked.
#pragma once
#include <hip/hip_runtime.h>

__device__ inline unsigned long long bl_splitmix(unsigned long long &x)
{
    unsigned long long z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct BlPredRng {
    unsigned s0, s1, s2, s3;
    __device__ BlPredRng(unsigned long long seed, unsigned long long index)
    {
        unsigned long long x = seed ^ (index * 0xD1342543DE82EF95ull);
        const unsigned long long a = bl_splitmix(x), b = bl_splitmix(x);
        s0 = (unsigned)a; s1 = (unsigned)(a >> 32); s2 = (unsigned)b; s3 = (unsigned)(b >> 32) | 1u;
    }
    __device__ float uniform() // [0, 1)
    {
        const unsigned r0 = s0 + s3, r = ((r0 << 7) | (r0 >> 25)) + s0, t = s1 << 9;
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t; s3 = (s3 << 11) | (s3 >> 21);
        return (float)(r >> 8) * 5.9604644775390625e-08f;
    }
};
// the generator of cell (draw n, period t of T, site i of N), n the absolute draw index
__device__ inline BlPredRng bl_cell_rng(unsigned long long seed, int n, int T, int t, int N, int i)
{
    return BlPredRng(seed, ((unsigned long long)n * T + t) * N + i);
}
// Binomial(n, p) as n Bernoulli trials, one uniform each: exact, and the number of uniforms is n whatever p is
// (nmixture's predictive counts, n <= 127; occu_cop's true detections among a visit's count)
__device__ inline int bl_binomial(BlPredRng &rng, int n, float p)
{
    int cnt = 0;
    for (int m = 0; m < n; m++) cnt += rng.uniform() < p ? 1 : 0;
    return cnt;
}
