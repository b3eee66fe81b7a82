"""predictive_check without a GPU: the export, the refusals and the argument checks -- all of them in front of any device call."""
import numpy as np
import pytest

from biolith_amd import models
from biolith_amd.evaluation import posterior_predictive_check


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((1, 4, 1, 2), np.float32))


def test_predictive_check_is_exported():
    from biolith_amd import utils
    from biolith_amd.utils import predictive_check

    assert "predictive_check" in utils.__all__ and callable(predictive_check)
    doc = predictive_check.__doc__
    assert "posterior_predictive_check(predict(" in doc and "without false positives" in doc


@pytest.mark.parametrize("name", ["occu_rn", "occu_cop", "nmixture", "occu_cs", "occu_comb", "occu_dyn"])
def test_other_models_are_refused_before_any_device_call(name):
    from biolith_amd.utils import predictive_check

    with pytest.raises(NotImplementedError, match=rf"predictive_check\(\): not built for {name} \(built: occu "):
        predictive_check(getattr(models, name), _NoPosterior(), **DATA)


def test_not_a_model_is_a_type_error():
    from biolith_amd.utils import predictive_check

    with pytest.raises(TypeError, match="biolith_amd model"):
        predictive_check(lambda **kw: None, _NoPosterior(), **DATA)


@pytest.mark.parametrize("bad", [dict(group_by="species"), dict(statistic="deviance")])
def test_bad_arguments_raise_the_host_checks_messages(bad):
    from biolith_amd.utils import predictive_check

    with pytest.raises(ValueError) as host:
        posterior_predictive_check({}, DATA["obs"], **bad)
    with pytest.raises(ValueError) as fused:
        predictive_check(models.occu, _NoPosterior(), **DATA, **bad)
    assert str(fused.value) == str(host.value)
