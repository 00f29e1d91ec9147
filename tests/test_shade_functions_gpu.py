"""The material functions, the f64 forms of precise shading and the tone-map curve ON THE DEVICE (v_rcp_f32, v_rsq_f32, v_sqrt_f32, v_sin / v_cos in
revolutions, v_exp / v_log — where the host emulation has libm), point by point against the f64 oracle: the sets, the sensitivity and the check
of tests/shade_sweeps.py through the gfx950 build of tests/shade_probe (made by __graft_entry__.build(); one launch of a few thousand threads
per test).  tests/test_shade_functions_cpu.py asserts the sets' conditions on the oracle alone and that the check rejects subtly wrong values.
Figures: profiles/shade_sweeps.txt."""
import pytest

import shade_sweeps as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_probe():
    return ss.load_device_probe()       # RuntimeError when the library is missing: no skip, no fall-back to the host build


@pytest.mark.parametrize("name", ss.SETS)
def test_point_set_on_the_device(device_probe, name):
    """Every point within max(T, K sens) of the oracle, finite where the oracle is, every decision the oracle's or the point fragile."""
    ss.check_set(device_probe, name, "MI355X")


def test_f64_forms_on_the_device(device_probe):
    ss.check_f64_forms(device_probe, "MI355X")


def test_post_curve_on_the_device(device_probe):
    ss.check_post(device_probe, "MI355X")
