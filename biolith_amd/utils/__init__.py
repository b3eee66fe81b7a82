from .abundance import conditional_abundance
from .dynamics import conditional_dynamics
from .fit import FitResult, fit
from .grid_search import GridSearchResult, grid_search_priors
from .information_criteria import information_criteria
from .init import init_to_feasible, init_to_mean, init_to_median, init_to_sample, init_to_uniform, init_to_value
from .latent import conditional_occupancy
from .loo import compare_marginal, loo_marginal
from .predict import predict
from .predict_comb import predict_comb
from .predictive_check import predictive_check
from .predictive_check_counts import predictive_check_counts
from .scores import conditional_scores
from .site_summary import site_summary
from .site_diagnostics import site_diagnostics
from .regional_totals import regional_totals
from .response_curves import response_curves
from .trajectory_totals import trajectory_totals
from .species_richness import species_richness
from .residual_moran import neighbour_graph, residual_moran
from .counts import conditional_counts

__all__ = ["fit", "FitResult", "predict", "predict_comb", "predictive_check", "predictive_check_counts", "information_criteria", "site_summary", "site_diagnostics", "regional_totals", "response_curves", "trajectory_totals", "species_richness", "residual_moran", "neighbour_graph", "conditional_occupancy", "conditional_abundance", "conditional_dynamics", "conditional_scores", "conditional_counts", "loo_marginal", "compare_marginal", "grid_search_priors", "GridSearchResult", "init_to_uniform", "init_to_feasible", "init_to_value",
           "init_to_mean", "init_to_median", "init_to_sample"]
