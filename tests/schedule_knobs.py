"""The schedule-only options of the device context, in one table.

How work is handed out never changes the image: every path leaves its radiance in its own hand-off record and accumulate_kernel sums a pixel's
records in a fixed order, so work-unit size, grid size, wave budget, priorities and queue layout are free to move.  KNOBS lists
every option that may only move those — tests/test_schedule_gpu.py renders each value of each row and compares with the render at the defaults,
bit for bit — and OTHER_OPTIONS lists every other key hr_set_option / hr_set_debug_option know, with the reason it is no row and the test that
covers it.  Both carry every key's setter and default (ALL_DEFAULTS, SETTERS: what tests/gpu_helpers.py's options() restores to).
tests/test_schedule_cpu.py reads the keys and the defaults out of hr_api.hip: a new option fails there until it is in one of the two.

No GPU in this module."""
from collections import namedtuple, OrderedDict

MEGA, SPLIT = 0, 1            # debug option trace_mode: the megakernel (trace_kernel) / the split pipeline (wf_kernels.h)
BOTH = (MEGA, SPLIT)
HUGE = 1000000                # more than any test frame has tiles, work units or workgroups

# key; "set_option" | "set_debug_option" (the Renderer method); the default (hr_ctx's initialiser in hr_api.hip); the pipelines whose launches
# read it; the edge values — `reduced` is the part of them that also runs on the strips and on the other scenes
Knob = namedtuple("Knob", "key setter default pipelines values reduced")

KNOBS = OrderedDict((k.key, k) for k in [
    # trace_kernel's work units (trace_kernel.h): samplings per unit — a launch of 3 samplings has num_k = 3 and the last one num_k = 1: 1, 2 (a
    # partial last chunk), 3 (= num_k), 5 (> num_k), 64
    Knob("kchunk", "set_debug_option", 0, (MEGA,), (1, 2, 3, 5, 64), (1, 5)),
    # the finer tail: off, every tile in the tail (bulk_units == 0), half, the default's neighbour, more than there are tiles (tail_tiles == 0)
    Knob("tail_div", "set_debug_option", 16, (MEGA,), (0, 1, 2, 16, HUGE), (1, HUGE)),
    # absolute grid: one workgroup, three, more than there are units (clamped by the unit count)
    Knob("trace_grid", "set_debug_option", 0, (MEGA,), (1, 3, HUGE), (1,)),
    Knob("trace_wgs", "set_debug_option", 6, (MEGA,), (1, 8), ()),
    # the wave budget, pinned: around the split pipeline's multiples of 16 workgroups (below 16 means 16 there), and more than the grid has
    Knob("trace_budget", "set_debug_option", 0, BOTH, (1, 2, 15, 16, 17, 31, 32, 33, HUGE), (1, 17)),
    # the phase thresholds of the walk (traverse_wave); the split pipeline's traversal kernel takes wf_adv_den for adv_den
    Knob("adv_den", "set_debug_option", 2, (MEGA,), (1, 64), ()),
    Knob("leaf_den", "set_debug_option", 2, BOTH, (1, 64), ()),
    Knob("node_unroll", "set_debug_option", 2, BOTH, (1,), ()),
    # s_setprio of the seed kernel's waves, and which kernel's waves come first (-1: governed on the device)
    Knob("seed_prio", "set_debug_option", 3, BOTH, (0, 1, 2, 3), ()),
    Knob("init_prio", "set_debug_option", 1, BOTH, (0, 1, 2, 3), ()),
    Knob("trace_boost", "set_option", -1, BOTH, (0, 1, 2, 3, 4), ()),
    # the split pipeline: when the traversal kernel leaves its walk, and the grids of its two kernels (workgroups per CU)
    Knob("wf_adv_den", "set_debug_option", 2, (SPLIT,), (0, 1, 64), ()),
    Knob("wf_trav_wgs", "set_debug_option", 8, (SPLIT,), (1, 16), (1,)),
    Knob("wf_shade_wgs", "set_debug_option", 8, (SPLIT,), (1, 16), (1,)),
])

DEFAULTS = OrderedDict((k.key, k.default) for k in KNOBS.values())
# the two combined settings: every knob at the small / the large end of what the library accepts
SMALLEST = OrderedDict([("kchunk", 1), ("tail_div", 1), ("trace_grid", 1), ("trace_wgs", 1), ("trace_budget", 1), ("adv_den", 1), ("leaf_den", 1),
                        ("node_unroll", 1), ("seed_prio", 0), ("init_prio", 0), ("trace_boost", 0), ("wf_adv_den", 0), ("wf_trav_wgs", 1), ("wf_shade_wgs", 1)])
LARGEST = OrderedDict([("kchunk", 64), ("tail_div", HUGE), ("trace_grid", HUGE), ("trace_wgs", 8), ("trace_budget", HUGE), ("adv_den", 64), ("leaf_den", 64),
                       ("node_unroll", 2), ("seed_prio", 3), ("init_prio", 3), ("trace_boost", 4), ("wf_adv_den", 64), ("wf_trav_wgs", 16), ("wf_shade_wgs", 16)])
COMBINED = OrderedDict([("smallest", SMALLEST), ("largest", LARGEST)])

# the knobs of the unit decomposition and the budget hand-shake: what the tile-mask test sweeps (the LIST forms of trace_kernel / wf_start_kernel)
UNIT_KNOBS = ("kchunk", "tail_div", "trace_grid", "trace_budget")
# hr_debug_path_log plans its own launch with no tail and no budget: the knobs that still reach it
PATH_LOG_KNOBS = ("adv_den", "leaf_den", "node_unroll", "wf_adv_den", "wf_trav_wgs", "wf_shade_wgs")


def settings(pipeline, full=True, keys=None, combined=True):
    """[(label, {key: value})]: one setting per value of every row that acts on `pipeline` (`full`: all values, else the reduced list; `keys`:
    these rows only), then the two combined settings.  A single-knob setting whose value is the default is left out: it is the reference."""
    out = []
    for k in KNOBS.values():
        if pipeline not in k.pipelines or (keys is not None and k.key not in keys):
            continue
        for v in (k.values if full else k.reduced):
            if v != k.default:
                out.append(("%s=%d" % (k.key, v), {k.key: v}))
    if combined:
        out += [(name, dict(s)) for name, s in COMBINED.items()]
    return out


# Every other key of hr_set_option / hr_set_debug_option: why it is no row above, the test that covers it, its setter and its default (hr_ctx's
# initialiser again; rng_window is fixed at the library's ISAAC_TAIL, the only value it takes).
#   axis     tests/test_schedule_gpu.py sets it itself: the sweeps run under both of its values (or with it on and off)
#   image    it changes the image, the tree or a plane, or what a later call does
#   variant  another instruction stream or another seed kernel for the same bits, pinned at full size by a test of its own
Other = namedtuple("Other", "kind covered_by setter default")
P, D = "set_option", "set_debug_option"

OTHER_OPTIONS = {key: Other(*row) for key, row in {
    "trace_mode": ("axis", "tests/test_schedule_gpu.py (every sweep, both values); test_gpu_parity.py::test_kernel_variants_render_the_same_bits", D, -1),
    "precise_shading": ("axis", "tests/test_schedule_gpu.py (every sweep, 0 and 1); test_gpu_parity.py::test_precise_shading_defaults_and_finite_radiance", P, -1),
    "counters": ("axis", "tests/test_schedule_gpu.py::test_accounting_sweep; test_gpu_parity.py::test_kernel_variants_render_the_same_bits", P, 0),
    "batch": ("image", "the fp32 accumulator depends on the launch cuts: test_gpu_parity.py::test_sharding_and_batching_are_exact_partitions", P, 0),
    "sample_counts": ("image", "a plane: tests/test_adaptive_gpu.py::test_counts", P, 0),
    "moments": ("image", "a plane: tests/test_moments_gpu.py", P, 0),
    "robust_buckets": ("image", "a plane: tests/test_robust_gpu.py", P, 0),
    "guide_bounces": ("image", "the guide planes: tests/test_guide_chain_gpu.py", P, 0),
    "russian_roulette": ("image", "another estimator: test_gpu_parity.py::test_russian_roulette_is_unbiased_and_off_by_default; "
                                  "tests/test_schedule_gpu.py::test_roulette_and_precise_shading_refuse_each_other", P, 0),
    "quant_nodes": ("image", "the tree's record format, next upload: test_gpu_parity.py::test_kernel_variants_render_the_same_bits", P, 1),
    "bvh_builder": ("image", "the tree: test_gpu_parity.py::test_device_bvh_build_is_interchangeable", P, -1),
    "max_leaf": ("image", "the tree: test_gpu_parity.py::test_device_bvh_build_is_interchangeable", P, 4),
    "split_ratio": ("image", "the tree: tests/test_bvh_edges_gpu.py", P, -1.0),
    "ploc_top": ("image", "the tree: tests/test_bvh_edges_gpu.py", D, 8192),
    "max_tail_gib": ("image", "caps the samplings per launch, i.e. the launch cuts: test_gpu_parity.py::test_config5_4k_crops", P, 20),
    "rng_window": ("image", "fixed in this build: test_gpu_parity.py::test_error_paths", P, 64),
    "nee_cull": ("image", "which shadow rays are traced (same accumulator, other ray counts): test_gpu_parity.py::test_nee_culls_do_not_change_a_bit", D, 7),
    "draw_residuals": ("image", "precise shading without the draws' residuals is another image: tests/test_seed_prerun.py", D, 1),
    "debug_skip": ("image", "a garbage image on purpose (timing experiments): test_gpu_parity.py::test_error_paths", D, 0),
    "seed_prof": ("image", "the seed kernel's timing build fills hr_stats.seed_phase_cycles: tests/test_adaptive_gpu.py (refused under a tile mask)", D, 0),
    "min_waves": ("variant", "test_gpu_parity.py::test_kernel_variants_render_the_same_bits", D, 5),
    "seed_mode": ("variant", "test_gpu_parity.py::test_seed_kernels_are_bit_identical, ::test_seed_kernels_agree_on_odd_shapes", D, 2),
    "seed_split": ("variant", "test_gpu_parity.py::test_seed_kernels_are_bit_identical", D, 16),
    "seed_prerun": ("variant", "tests/test_seed_prerun.py", D, 1),
}.items()}

def split(setting):
    """(options, debug options) of a setting: what gpu_helpers.options takes"""
    return tuple({k: v for k, v in setting.items() if SETTERS[k] == setter} for setter in (P, D))


# every option's default and setter, the knobs and the others together: what tests/gpu_helpers.py's options() restores to, and through what
ALL_DEFAULTS = dict(DEFAULTS, **{key: o.default for key, o in OTHER_OPTIONS.items()})
SETTERS = dict({k.key: k.setter for k in KNOBS.values()}, **{key: o.setter for key, o in OTHER_OPTIONS.items()})
