"""Region rendering (hr_set_region) on the CPU tier: the entry points are declared, exported and bound by every host layer, and the
CLI's --region is documented and checked before any device is opened."""
import ctypes as C
import os
import re

import pytest

from cli import run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _product_header():
    text = open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_region_entry_points_declared_and_exported(ha):
    text = _product_header()
    assert re.search(r"int\s+hr_set_region\s*\(\s*hr_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", text)
    assert re.search(r"int\s+hr_get_region\s*\(\s*hr_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\[\s*4\s*\]\s*\)\s*;", text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7   # only functions were added
    lib = C.CDLL(ha.HIP_LIB)
    assert hasattr(lib, "hr_set_region") and hasattr(lib, "hr_get_region")


def test_rust_mirror_binds_the_region():
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    assert re.search(r"pub fn hr_set_region\(ctx: \*mut HrCtx, x0: u32, y0: u32, w: u32, h: u32\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_get_region\(ctx: \*mut HrCtx, out_xywh: \*mut u32", ffi)
    ren = open(os.path.join(ROOT, "rust", "hip_renderer.rs")).read()
    assert "hr_set_region(self.ctx" in ren and "pub region: Option<(u32, u32, u32, u32)>" in ren


def test_python_renderer_has_set_region(ha):
    assert callable(getattr(ha.Renderer, "set_region", None)) and callable(getattr(ha.Renderer, "region", None))
    L = ha.hip_lib()
    assert L.hr_set_region.argtypes is not None and len(L.hr_set_region.argtypes) == 5


def test_cli_help_lists_region(tmp_path):
    r = run_cli(["--help"], tmp_path, missing="skip")
    assert r.returncode == 0 and "--region X,Y,W,H" in r.stdout


@pytest.mark.parametrize("args", [["--region", "10,10,0,5"], ["--region", "470,0,20,5", "-w", "480", "-h", "270"],
                                  ["--region", "0,0,481,1", "-w", "480", "-h", "270"], ["--region", "4294967295,0,2,1", "-w", "480", "-h", "270"],
                                  ["--region", "1,2,3"], ["--region", "1,2,3,4,5"], ["--region", "-1,0,4,4"], ["--region", "1,2,3,x"]])
def test_cli_rejects_a_bad_region_before_any_device(tmp_path, args):
    """Malformed or out-of-frame windows are argument errors: exit status 1 and a message naming --region, before the log file is opened
    or a device is touched (no result.txt; on a machine without a GPU no device error either)."""
    r = run_cli(args, tmp_path, missing="skip")
    assert r.returncode == 1, r.stdout
    assert "--region" in r.stdout
    assert not (tmp_path / "result.txt").exists()
