"""What the plumbing checks of the feature tests share: the product header without its comments, the pattern of a context argument, the exported
symbols, the Rust and INTEGRATION.md texts, and the CLI run that must be refused.  Each test keeps its own patterns, names, counts and words.

No GPU in this module."""
import ctypes as C
import os
import re

from cli import run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX = r"hr_ctx\s*\*\s*\w*"


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def header_text(raw=False):
    """include/hanamaru_hip.h, by default with its comments stripped"""
    text = read("include", "hanamaru_hip.h")
    return text if raw else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(text, regex):
    """the declaration matching regex, with %s standing for a context argument"""
    return re.search(regex.replace("%s", CTX), text)


def abi_version(text):
    return int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1))


def exported_and_bound(ha, names):
    """the names among `names` that the HIP library, opened afresh, does not export (none: an empty list)"""
    lib = C.CDLL(ha.HIP_LIB)
    return [n for n in names if not hasattr(lib, n)]


def rust_ffi():
    return read("rust", "hip_ffi.rs")


def kernel_variants():
    return read("hanamaru-renderer_amd", "csrc", "kernel_variants.h")


def cli_refused(tmp_path, args, size=("-w", "64", "-h", "48", "-s", "8"), **kw):
    """the CLI run with a small frame and args, which must end before any device is opened: (the finished run, whether it left a result file)"""
    r = run_cli(list(size) + args, tmp_path, **kw)
    return r, (tmp_path / "result.txt").exists()
