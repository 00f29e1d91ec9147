"""Sharded statistics on the CPU tier: the two entry points and the option declared, documented, exported and bound; the ABI
version unchanged; the kernel rows of the by-sampling bucket form beside the untouched ordinal ones; the fold kernel's shape in the source."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_functions_and_documents_the_option():
    raw = _read("include", "hanamaru_hip.h")
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+hr_fold_statistics\s*\(\s*hr_ctx\s*\*\s*\w*\s*\)\s*;", code)
    assert re.search(r"int\s+hr_fold_statistics_group\s*\(\s*hr_ctx\s*\*\*\s*\w*\s*,\s*int\s+\w*\s*\)\s*;", code)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", code).group(1)) == 7       # functions and one option were added, no struct changed
    comments = " ".join(re.findall(r"/\*.*?\*/", raw, flags=re.S))
    assert comments.count('"bucket_by_sampling"') >= 3                                     # the contract, the refusal and the option list
    for phrase in ("(s - 1) mod K", "samplings 1 .. n", "HR_COMM_SAME_DEVICE_SUM", "ncclReduce", "post_kernel_ms", "HR_ERR_NO_TARGET", "HR_ERR_UNSUPPORTED",
                   "A group of one"):
        assert phrase in comments, phrase
    assert "no library-side collective" not in re.sub(r"\s+\*?\s*", " ", raw)             # the three remarks the fold made untrue


def test_library_exports_and_python_binds_both_entry_points(ha):
    lib = C.CDLL(ha.HIP_LIB)
    assert hasattr(lib, "hr_fold_statistics") and hasattr(lib, "hr_fold_statistics_group")
    assert callable(getattr(ha.Renderer, "fold_statistics", None)) and callable(getattr(ha, "fold_statistics", None))
    src = _read("hanamaru-renderer_amd", "python", "hanamaru_amd", "__init__.py")
    assert re.search(r"L\.hr_fold_statistics\.argtypes = \[C\.c_void_p\]", src)
    assert re.search(r"L\.hr_fold_statistics_group\.argtypes = \[C\.POINTER\(C\.c_void_p\), C\.c_int\]", src)
    assert re.search(r"def fold_statistics\(self\):.*?self\.L\.hr_fold_statistics\(self\._h\)", src, re.S)
    assert re.search(r"\ndef fold_statistics\(renderers\):.*?L\.hr_fold_statistics_group\(arr, len\(renderers\)\)", src, re.S)


def test_rust_mirror_and_integration_guide_are_in_step():
    for text in (_read("rust", "hip_ffi.rs"), _read("INTEGRATION.md")):
        assert re.search(r"pub fn hr_fold_statistics\(ctx: \*mut HrCtx\) -> c_int;", text)
        assert re.search(r"pub fn hr_fold_statistics_group\(ctxs: \*mut \*mut HrCtx, n: c_int\) -> c_int;", text)


def test_bucket_kernel_rows():
    kv = _read("hanamaru-renderer_amd", "csrc", "kernel_variants.h")
    # the ordinal rows as they were, and the same three launches by sampling: uniform, sample_counts on, a tile mask
    for row in ("HR_VARIANT(bucket_kernel, false, false)", "HR_VARIANT(bucket_kernel, true, false)", "HR_VARIANT(bucket_kernel, true, true)",
                "HR_VARIANT(bucket_kernel, false, false, true)", "HR_VARIANT(bucket_kernel, true, false, true)", "HR_VARIANT(bucket_kernel, true, true, true)"):
        assert kv.count(row) == 1, row
    assert re.search(r"select_bucket_kernel\(bool counts, bool list, bool by_sampling\)", kv)
    tk = _read("hanamaru-renderer_amd", "csrc", "trace_kernel.h")
    assert re.search(r"template <bool CNTS, bool LIST = false, bool BYS = false>\s*__global__ __launch_bounds__\(256\) void bucket_kernel", tk)


def test_fold_kernel_and_reduce_in_the_source():
    api = _read("hanamaru-renderer_amd", "csrc", "hr_api.hip")
    body = re.search(r"void fold_plane_kernel\(.*?\n}\n", api, re.S).group(0)
    assert "atomic" not in body
    for vec in ("double2", "float4", "uint4"):
        assert re.search(r"FoldVec<\w+> \{ typedef %s type; \}" % vec, api), vec
    assert re.search(r"std::min<size_t>\(2048,", api)                                     # the capped grid of the memory-bound idiom
    comm = _read("hanamaru-renderer_amd", "csrc", "hr_comm.h")
    assert 'sym("ncclReduce")' in comm
    for code in ("kFloat = 7", "kUint32 = 3", "kUint64 = 5", "kDouble = 8"):              # ncclFloat32, ncclUint32, ncclUint64, ncclFloat64
        assert code in comm, code


def test_the_option_has_its_default_its_setter_and_a_test_that_covers_it():
    """What tests/schedule_knobs.py's OTHER_OPTIONS records for an option that changes a plane, held for "bucket_by_sampling" here: the default is
    hr_ctx's initialiser (0), it is an hr_set_option key and no debug key, it takes 0 and 1 only, and the GPU test that covers it exists."""
    api = _read("hanamaru-renderer_amd", "csrc", "hr_api.hip")
    ctx = re.search(r"\nstruct hr_ctx \{\n(.*?)\n\};", api, re.S).group(1)
    assert re.search(r"\bbool bucket_by_sampling = false;", ctx)
    setter = re.search(r"\nstatic bool set_sharding_option\(.*?\n}\n", api, re.S).group(0)
    assert 'key != "bucket_by_sampling"' in setter and "value != 0 && value != 1" in setter and "HR_ERR_INVALID" in setter
    product = re.search(r"\nint hr_set_option\(hr_ctx \*c, const char \*key, double value\) \{\n(.*?)\n\}\n", api, re.S).group(1)
    debug = re.search(r"\nint hr_set_debug_option\(hr_ctx \*c, const char \*key, double value\) \{\n(.*?)\n\}\n", api, re.S).group(1)
    assert "set_sharding_option(c, k, value, rc)" in product and "set_sharding_option" not in debug
    gpu = _read("tests", "test_fold_gpu.py")
    assert re.search(r"^def test_by_sampling_equals_ordinal_on_one_context\(", gpu, re.M) and 'set_option("bucket_by_sampling", by_sampling)' in gpu
