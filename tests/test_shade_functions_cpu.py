"""The material functions, the f64 forms of precise shading and the tone-map curve, asked point by point against the f64 oracle
(tests/shade_sweeps.py) — CPU tier: the conditions the point sets must meet on the oracle alone, every set through the g++ build of
tests/shade_probe (libm where the device has v_rcp / v_rsq / v_sin / v_exp: tests/test_shade_functions_gpu.py asks the device), and deliberately
wrong EXPECTED values that the check must reject.  Figures of both tiers: profiles/shade_sweeps.txt."""
import numpy as np
import pytest

import shade_sweeps as ss


@pytest.fixture(scope="session")
def host_probe(tmp_path_factory):
    return ss.build_host_probe(tmp_path_factory.mktemp("shade_probe"))


@pytest.mark.parametrize("name", ss.SETS)
def test_point_set_meets_its_conditions_on_the_oracle_alone(name):
    """A few thousand points; at most 1 % fragile; in the general sets K sens exceeds T at no more than 10 %; the oracle finite everywhere but in
    eval_rough0 (counted and printed)."""
    p = ss.get(name)
    fig = ss.oracle_conditions(p)
    print(name, fig)
    n = len(p["ref"])
    assert len(p["sens"]) == n and len(p["fragile"]) == n and len(p["decision"]) == n        # no point is left out
    assert np.isfinite(p["sens"][np.isfinite(p["ref"]).all(axis=1)]).all()
    if name == "eval_rough0":
        assert 0 < fig["oracle_not_finite"] < n // 2
    if name == "eval_grazing":
        assert 0 < p["zero_expected"].sum() < n // 50


@pytest.mark.parametrize("name", ss.SETS)
def test_point_set_on_the_host_build(host_probe, name):
    ss.check_set(host_probe, name, "host build")


def test_f64_forms_on_the_host_build(host_probe):
    ss.check_f64_forms(host_probe, "host build")


def test_post_curve_on_the_host_build(host_probe):
    ss.check_post(host_probe, "host build")


# ------------------------------------------------------------------------------------------------------------------------------------------
# the check has teeth: a subtly wrong EXPECTED value is rejected on the general sets, the code under test untouched
def _with_expected(p, ref):
    q = dict(p)
    q["ref"] = ref
    q["den"] = ss.floors(p, ref)
    return q


def test_numpy_bsdf_is_the_oracles():
    p = ss.get("eval_general")
    mine = ss.numpy_bsdf(p)
    assert np.abs(mine - p["ref"][:, 0]).max() <= 1e-9 * np.maximum(1.0, np.abs(p["ref"][:, 0])).max()


@pytest.mark.parametrize("variant", [{"schlick_exponent": 4}, {"inv_pi": (1.0 + 1e-4) / np.pi}, {"alpha_power": 1}])
def test_bsdf_eval_check_rejects_a_wrong_expected_value(host_probe, variant):
    """SENSITIVE: Schlick's exponent 4 for 5, 1 / pi off by 1e-4 of itself, alpha for alpha2."""
    p = ss.get("eval_general")
    got, dec = ss.run_probe(host_probe, p)
    fig, fails = ss.check(_with_expected(p, ss.numpy_bsdf(p, **variant)[:, None]), got, dec, "wrong expected value %s" % variant)
    print(ss.report_line(fig))
    assert fig["failures"] >= 100, fig


def test_bsdf_sample_check_rejects_a_wrong_expected_value(host_probe):
    """SENSITIVE: alpha for alpha2 in the expected GGX lobes (the oracle asked with sqrt(roughness)), and an offset of 1.5e-4 for 1e-4 (5e-5 of a position within the unit ball)."""
    p = ss.get("sample_general")
    got, dec = ss.run_probe(host_probe, p)
    q = dict(p)
    q["roughness"] = np.sqrt(p["roughness"].astype(np.float64)).astype(np.float32)
    wrong, _ = ss.oracle_outputs(q)
    fig, fails = ss.check(_with_expected(p, wrong), got, dec, "alpha for alpha2")
    print(ss.report_line(fig))
    rough_lobes = np.isin(p["surface"], (ss.GGX, ss.GGX_REFRACTION)) & (p["roughness"] < 1.0)
    assert fig["failures"] >= rough_lobes.sum() // 2, (fig, int(rough_lobes.sum()))
    wrong = p["ref"].copy()
    pos = p["pos"].astype(np.float64)
    wrong[:, 3:6] = pos + (p["ref"][:, 3:6] - pos) * 1.5
    near = np.sqrt((pos * pos).sum(-1)) < 1.0
    fig, fails = ss.check(_with_expected(p, wrong), got, dec, "offset 1.5e-4")
    print(ss.report_line(fig))
    assert fig["failures"] >= near.sum() // 2 > 100, (fig, int(near.sum()))


def test_f64_and_post_checks_reject_a_wrong_expected_value(host_probe):
    """SENSITIVE: 1e-12 of the expected f64 values (T64 = 1e-13), 1e-4 of the expected tone-mapped values (T = 1e-5)."""
    with pytest.raises(AssertionError):
        ss.check_f64_forms(host_probe, "expected values off by 1e-12", skew=1e-12)
    with pytest.raises(AssertionError):
        ss.check_post(host_probe, "expected values off by 1e-4", skew=1e-4)
