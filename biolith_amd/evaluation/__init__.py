from .diagnostics import diagnostics, effective_sample_size, split_gelman_rubin, summary
from .marginal_density import expected_true_detections, expected_true_positives, finite_sample_abundance, finite_sample_occupancy, finite_sample_turnover, lppd_marginal, waic_marginal
from .predictive_checks import deviance, deviance_manual, posterior_predictive_check, posterior_predictive_check_counts, residuals
from .predictive_density import log_likelihood, log_likelihood_comb, log_likelihood_manual, lppd, lppd_manual, waic, waic_comb, waic_manual

__all__ = ["diagnostics", "effective_sample_size", "split_gelman_rubin", "summary",
           "log_likelihood", "log_likelihood_manual", "lppd", "lppd_manual", "waic", "waic_manual", "log_likelihood_comb", "waic_comb",
           "lppd_marginal", "waic_marginal", "finite_sample_occupancy", "finite_sample_abundance", "finite_sample_turnover", "expected_true_positives", "expected_true_detections",
           "deviance", "deviance_manual", "posterior_predictive_check", "posterior_predictive_check_counts", "residuals"]
