// kernel_variants.h — which instantiation of a kernel family a launch runs.  One table per family and one select_*() beside it:
//   * a row names an instantiation ONCE (HR_VARIANT spells the template arguments as the row's key and as the function),
//   * select_*() turns the run-time facts of a launch (options, the scene's record format, the query that launches) into a key and looks the
//     row up — the quirks of that mapping are written there and nowhere else; nullptr: the table has no such row, the caller refuses,
//   * create_resources (hr_api.hip) walks the same tables: the LDS attribute of every seed kernel, the "no LDS" guard of every trace-side
//     kernel.  What a launch can run is a row, so both loops have seen it.
// A new variant is a new row (and a line in its selector if a new fact selects it); nothing else spells a <...> list of these kernels.
// No row for a combination that is never launched: every trace_kernel instantiation costs compile time and code-object size.
// Included by hr_api.hip behind the kernel headers (one translation unit; the kernels are static to it).
#pragma once

#define HR_VARIANT(kernel, ...) {__VA_ARGS__, kernel<__VA_ARGS__>}
template <class Row, size_t N, class Match>
static const Row *find_row(const Row (&table)[N], Match match) {
    for (const Row &r : table)
        if (match(r)) return &r;
    return nullptr;
}
template <class Row>
static auto fn_of(const Row *r) -> decltype(r->fn) { return r ? r->fn : nullptr; }   // nullptr: no such row

// ---- trace_kernel<CNT, MINW, QN, RR, LOG, PREC, LIST> (trace_kernel.h) ----
typedef void (*TraceFn)(Scene, RenderParams, float *, Counters *, uint32_t *, uint32_t *);
struct TraceVariant { bool cnt; int minw; bool qn, rr, log, prec, list; TraceFn fn; };
static const TraceVariant TRACE_VARIANTS[] = {
    // fp32 shading: the default (5 waves), the tree of 32-byte nodes, debug option min_waves 4 / 6, the counters build
    HR_VARIANT(trace_kernel, false, 5, true, false, false, false, false), HR_VARIANT(trace_kernel, false, 5, false, false, false, false, false),
    HR_VARIANT(trace_kernel, false, 4, true, false, false, false, false), HR_VARIANT(trace_kernel, false, 6, true, false, false, false, false),
    HR_VARIANT(trace_kernel, true, 3, true, false, false, false, false), HR_VARIANT(trace_kernel, true, 3, false, false, false, false, false),
    // the roulette estimator (option russian_roulette)
    HR_VARIANT(trace_kernel, false, 5, true, true, false, false, false), HR_VARIANT(trace_kernel, false, 5, false, true, false, false, false),
    HR_VARIANT(trace_kernel, true, 3, true, true, false, false, false), HR_VARIANT(trace_kernel, true, 3, false, true, false, false, false),
    // precise shading (path_advance<.., PREC>): 128 VGPRs, debug option min_waves 6 -> the 96-VGPR form, 4 -> the 168-VGPR form, the counters build
    HR_VARIANT(trace_kernel, false, 4, true, false, false, true, false), HR_VARIANT(trace_kernel, false, 4, false, false, false, true, false),
    HR_VARIANT(trace_kernel, false, 5, true, false, false, true, false), HR_VARIANT(trace_kernel, false, 3, true, false, false, true, false),
    HR_VARIANT(trace_kernel, true, 3, true, false, false, true, false), HR_VARIANT(trace_kernel, true, 3, false, false, false, true, false),
    // the path log (hr_debug_path_log)
    HR_VARIANT(trace_kernel, false, 3, true, false, true, false, false), HR_VARIANT(trace_kernel, false, 3, false, false, true, false, false),
    HR_VARIANT(trace_kernel, false, 3, true, false, true, true, false), HR_VARIANT(trace_kernel, false, 3, false, false, true, true, false),
    // a tile mask is in force (hr_set_tile_mask / hr_select_tiles, adapt_core.h): the default fp32 and precise forms over the active-tile list
    HR_VARIANT(trace_kernel, false, 5, true, false, false, false, true), HR_VARIANT(trace_kernel, false, 5, false, false, false, false, true),
    HR_VARIANT(trace_kernel, false, 4, true, false, false, true, true), HR_VARIANT(trace_kernel, false, 4, false, false, false, true, true),
};
// counters / qn (the scene has quantised nodes) / rr (rr_start != 0) / precise / min_waves as the context has them; log: the path log's launch.
//   * the log builds are one occupancy form (MINW 3) and know neither counters nor roulette
//   * the roulette estimator ignores min_waves (and has no f64 form: hr_render refuses the pair)
//   * counters builds are MINW 3 whatever min_waves says
//   * precise: min_waves 6 -> MINW 5, 4 -> MINW 3, otherwise MINW 4 — with quantised nodes only; without them MINW 4
//   * fp32: min_waves is MINW — with quantised nodes only; without them <false, 5, false>
//   * list (a tile mask is in force): the default occupancy forms only — no counters, roulette, path log, or min_waves other than 5
static TraceFn select_trace_kernel(bool counters, bool qn, bool rr, bool precise, int min_waves, bool log, bool list = false) {
    bool cnt = counters, prec = precise;
    int minw;
    if (log) { cnt = false; rr = false; minw = 3; }
    else if (rr) { prec = false; minw = cnt ? 3 : 5; }
    else if (cnt) minw = 3;
    else if (prec) minw = !qn ? 4 : min_waves == 6 ? 5 : min_waves == 4 ? 3 : 4;
    else minw = !qn ? 5 : min_waves == 4 ? 4 : min_waves == 6 ? 6 : 5;
    if (list && (cnt || rr || log || min_waves != 5)) return nullptr;
    return fn_of(find_row(TRACE_VARIANTS, [&](const TraceVariant &r) { return r.cnt == cnt && r.minw == minw && r.qn == qn && r.rr == rr && r.log == log && r.prec == prec && r.list == list; }));
}

// ---- the split pipeline (wf_kernels.h) ----
typedef void (*WfStartFn)(Scene, RenderParams, float *, WfQueues);
struct WfStartVariant { bool prec, list; WfStartFn fn; };   // list: a tile mask is in force (adapt_core.h)
static const WfStartVariant WF_START_VARIANTS[] = {HR_VARIANT(wf_start_kernel, false, false), HR_VARIANT(wf_start_kernel, true, false),
                                                   HR_VARIANT(wf_start_kernel, false, true), HR_VARIANT(wf_start_kernel, true, true)};
static WfStartFn select_wf_start_kernel(bool precise, bool list = false) {
    return fn_of(find_row(WF_START_VARIANTS, [&](const WfStartVariant &r) { return r.prec == precise && r.list == list; }));
}

typedef void (*WfTraverseFn)(Scene, RenderParams, WfQueues, uint32_t, Counters *);
struct WfTraverseVariant { bool cnt, qn; WfTraverseFn fn; };
static const WfTraverseVariant WF_TRAVERSE_VARIANTS[] = {HR_VARIANT(wf_traverse_kernel, false, true), HR_VARIANT(wf_traverse_kernel, false, false),
                                                         HR_VARIANT(wf_traverse_kernel, true, true), HR_VARIANT(wf_traverse_kernel, true, false)};
typedef void (*WfShadeFn)(Scene, RenderParams, float *, WfQueues, uint32_t, Counters *, uint32_t *);
struct WfShadeVariant { bool cnt, prec, log; WfShadeFn fn; };
static const WfShadeVariant WF_SHADE_VARIANTS[] = {HR_VARIANT(wf_shade_kernel, false, false, false), HR_VARIANT(wf_shade_kernel, false, true, false),
                                                   HR_VARIANT(wf_shade_kernel, true, false, false),  HR_VARIANT(wf_shade_kernel, true, true, false),
                                                   HR_VARIANT(wf_shade_kernel, false, false, true),  HR_VARIANT(wf_shade_kernel, false, true, true)};
// log: the path log's launch — it does not count, in either kernel (the traversal kernel has no log form of its own)
static WfTraverseFn select_wf_traverse_kernel(bool counters, bool qn, bool log) {
    const bool cnt = counters && !log;
    return fn_of(find_row(WF_TRAVERSE_VARIANTS, [&](const WfTraverseVariant &r) { return r.cnt == cnt && r.qn == qn; }));
}
static WfShadeFn select_wf_shade_kernel(bool counters, bool precise, bool log) {
    const bool cnt = counters && !log;
    return fn_of(find_row(WF_SHADE_VARIANTS, [&](const WfShadeVariant &r) { return r.cnt == cnt && r.prec == precise && r.log == log; }));
}

// ---- debug_render_kernel<CNT, QN> and trace_debug_kernel<QN, CNT> (trace_kernel.h): neither runs beside a seed kernel ----
typedef void (*DebugRenderFn)(Scene, RenderParams, int, float *, Counters *);
struct DebugRenderVariant { bool cnt, qn; DebugRenderFn fn; };
static const DebugRenderVariant DEBUG_RENDER_VARIANTS[] = {HR_VARIANT(debug_render_kernel, false, true), HR_VARIANT(debug_render_kernel, false, false),
                                                           HR_VARIANT(debug_render_kernel, true, true), HR_VARIANT(debug_render_kernel, true, false)};
static DebugRenderFn select_debug_render_kernel(bool counters, bool qn) {
    return fn_of(find_row(DEBUG_RENDER_VARIANTS, [&](const DebugRenderVariant &r) { return r.cnt == counters && r.qn == qn; }));
}
// ---- guide_render_kernel<QN> (trace_kernel.h): the denoiser's guide planes, one row per node format; runs beside nothing ----
typedef void (*GuideRenderFn)(Scene, RenderParams, float *);
struct GuideRenderVariant { bool qn; GuideRenderFn fn; };
static const GuideRenderVariant GUIDE_RENDER_VARIANTS[] = {HR_VARIANT(guide_render_kernel, true), HR_VARIANT(guide_render_kernel, false)};
static GuideRenderFn select_guide_render_kernel(bool qn) {
    return fn_of(find_row(GUIDE_RENDER_VARIANTS, [&](const GuideRenderVariant &r) { return r.qn == qn; }));
}
// ---- guide_chain_kernel<QN> (trace_kernel.h): the guide planes at the first non-delta hit (option guide_bounces > 0); 0 bounces is the kernel above ----
typedef void (*GuideChainFn)(Scene, RenderParams, uint32_t, float *);
struct GuideChainVariant { bool qn; GuideChainFn fn; };
static const GuideChainVariant GUIDE_CHAIN_VARIANTS[] = {HR_VARIANT(guide_chain_kernel, true), HR_VARIANT(guide_chain_kernel, false)};
static GuideChainFn select_guide_chain_kernel(bool qn) {
    return fn_of(find_row(GUIDE_CHAIN_VARIANTS, [&](const GuideChainVariant &r) { return r.qn == qn; }));
}
// ---- guide_lens_kernel<QN> (trace_kernel.h): the chain averaged over the lens points of hr_render_guides_lens, one row per node format ----
typedef void (*GuideLensFn)(Scene, RenderParams, uint32_t, uint32_t, float *);
struct GuideLensVariant { bool qn; GuideLensFn fn; };
static const GuideLensVariant GUIDE_LENS_VARIANTS[] = {HR_VARIANT(guide_lens_kernel, true), HR_VARIANT(guide_lens_kernel, false)};
static GuideLensFn select_guide_lens_kernel(bool qn) {
    return fn_of(find_row(GUIDE_LENS_VARIANTS, [&](const GuideLensVariant &r) { return r.qn == qn; }));
}
// ---- motion_kernel<QN> (trace_kernel.h): the motion plane of hr_render_motion, one row per node format ----
typedef void (*MotionFn)(Scene, RenderParams, ReprojectCam, float, float, float *);
struct MotionVariant { bool qn; MotionFn fn; };
static const MotionVariant MOTION_VARIANTS[] = {HR_VARIANT(motion_kernel, true), HR_VARIANT(motion_kernel, false)};
static MotionFn select_motion_kernel(bool qn) {
    return fn_of(find_row(MOTION_VARIANTS, [&](const MotionVariant &r) { return r.qn == qn; }));
}
typedef void (*TraceDebugFn)(Scene, RenderParams, uint32_t, const float *, const float *, float *, int32_t *, Counters *);
struct TraceDebugVariant { bool qn, cnt; TraceDebugFn fn; };
static const TraceDebugVariant TRACE_DEBUG_VARIANTS[] = {HR_VARIANT(trace_debug_kernel, true, false), HR_VARIANT(trace_debug_kernel, false, false),
                                                         HR_VARIANT(trace_debug_kernel, true, true), HR_VARIANT(trace_debug_kernel, false, true)};
static TraceDebugFn select_trace_debug_kernel(bool counters, bool qn) {
    return fn_of(find_row(TRACE_DEBUG_VARIANTS, [&](const TraceDebugVariant &r) { return r.cnt == counters && r.qn == qn; }));
}

// ---- the seed kernels (seed_kernels.h) ----
// Every one takes (rp, lens_shape, [ring,] recs, ovf, win, counters) and SEED_LDS_BYTES of dynamic LDS; `ring`: it has the ring argument.
// key: mode = option seed_mode; split = init blocks of the producer waves (seed_pc_kernel only, else 0); prof = the phase-timing build (a
// number for seed_ps_kernel, else 0 / 1); lo = the launch writes the draws' residuals into the records' twin (seed_seg_kernel only);
// list = a tile mask is in force (adapt_core.h; the last member: seed_seg_kernel without its timing build only).
// pre = the pre-run form of seed_seg_kernel's window (debug option seed_prerun, the default; false everywhere else).
struct SeedVariant { int mode, split, prof; bool lo; const void *fn; uint32_t threads; bool ring; bool list = false; bool pre = false; };
static const SeedVariant SEED_VARIANTS[] = {
    {0, 0, 0, false, (const void *)seed_isaac64_kernel, 64 * SEED_WAVES, false},
    {1, 8, 0, false, (const void *)seed_pc_kernel<8>, 256, true},
    {1, 12, 0, false, (const void *)seed_pc_kernel<12>, 256, true},
    {1, 16, 0, false, (const void *)seed_pc_kernel<16>, 256, true},
    {1, 20, 0, false, (const void *)seed_pc_kernel<20>, 256, true},
    {1, 24, 0, false, (const void *)seed_pc_kernel<24>, 256, true},
    {1, 28, 0, false, (const void *)seed_pc_kernel<28>, 256, true},
    {1, 16, 1, false, (const void *)seed_pc_kernel<16, true>, 256, true},
    {1, 20, 1, false, (const void *)seed_pc_kernel<20, true>, 256, true},
    {2, 0, 0, false, (const void *)seed_seg_kernel<false, false>, 256, true},
    {2, 0, 1, false, (const void *)seed_seg_kernel<true, false>, 256, true},
    {2, 0, 0, true, (const void *)seed_seg_kernel<false, true>, 256, true},
    {2, 0, 1, true, (const void *)seed_seg_kernel<true, true>, 256, true},
    {2, 0, 0, false, (const void *)seed_seg_kernel<false, false, true>, 256, true, true},
    {2, 0, 0, true, (const void *)seed_seg_kernel<false, true, true>, 256, true, true},
    {2, 0, 2, false, (const void *)seed_seg_kernel<2, false>, 256, true},                           // seed_prof 2: the producer waves' timing
    // the same rows in the pre-run form
    {2, 0, 0, false, (const void *)seed_seg_kernel<false, false, false, true>, 256, true, false, true},
    {2, 0, 1, false, (const void *)seed_seg_kernel<true, false, false, true>, 256, true, false, true},
    {2, 0, 0, true, (const void *)seed_seg_kernel<false, true, false, true>, 256, true, false, true},
    {2, 0, 1, true, (const void *)seed_seg_kernel<true, true, false, true>, 256, true, false, true},
    {2, 0, 0, false, (const void *)seed_seg_kernel<false, false, true, true>, 256, true, true, true},
    {2, 0, 0, true, (const void *)seed_seg_kernel<false, true, true, true>, 256, true, true, true},
    {2, 0, 2, false, (const void *)seed_seg_kernel<2, false, false, true>, 256, true, false, true},
#if defined(HR_EXPERIMENTS)
    {3, 0, 0, false, (const void *)seed_ps_kernel<0>, 256, true},
    {3, 0, 1, false, (const void *)seed_ps_kernel<1>, 256, true},
    {3, 0, 2, false, (const void *)seed_ps_kernel<2>, 256, true},
    {3, 0, 3, false, (const void *)seed_ps_kernel<3>, 256, true},
    {4, 0, 0, false, (const void *)seed_w5_kernel<false>, 320, true},
    {4, 0, 1, false, (const void *)seed_w5_kernel<true>, 320, true},
#endif
};
// seed_mode / seed_split / seed_prof as the context has them; twin: the launch carries the residual twin (rp.rec_lo_off != 0).
//   * only the three-run kernel (mode 2) writes the twin
//   * the ring kernel (mode 1): its phase-timing build exists for splits 16 and 20 only and falls back to 16
//   * seed_ps_kernel (mode 3) has timing builds 1 .. 3, any other seed_prof is its plain build; everywhere else seed_prof is on / off
//   * the fused kernel (mode 0) has no timing build
//   * list (a tile mask is in force): the three-run kernel (mode 2) without phase timing, nothing else
//   * the three-run kernel (mode 2) alone has the pre-run form (seed_prerun) and a timing build of its producer waves (seed_prof 2, without the twin)
static const SeedVariant *select_seed_kernel(int seed_mode, int seed_split, int seed_prof, bool twin, bool list = false, bool prerun = false) {
    int split = 0, prof = seed_prof ? 1 : 0;
    bool lo = false, pre = false;
    if (seed_mode == 2) { lo = twin; pre = prerun; if (seed_prof == 2) prof = 2; }
    else if (seed_mode == 1) split = prof ? (seed_split == 20 ? 20 : 16) : seed_split;
    else if (seed_mode == 3) prof = seed_prof >= 1 && seed_prof <= 3 ? seed_prof : 0;
    else if (seed_mode == 0) prof = 0;
    return find_row(SEED_VARIANTS, [&](const SeedVariant &r) { return r.mode == seed_mode && r.split == split && r.prof == prof && r.lo == lo && r.list == list && r.pre == pre; });
}

// ---- accumulate_kernel<MOM, CNTS, LIST> (trace_kernel.h): a launch's radiance into the accumulator ----
typedef void (*AccumulateFn)(RenderParams, const float *, float *, double *, uint32_t *);
struct AccumulateVariant { bool mom, cnts, list; AccumulateFn fn; };
static const AccumulateVariant ACCUMULATE_VARIANTS[] = {HR_VARIANT(accumulate_kernel, false, false, false), HR_VARIANT(accumulate_kernel, true, false, false),
                                                        HR_VARIANT(accumulate_kernel, false, true, false),  HR_VARIANT(accumulate_kernel, true, true, false),
                                                        HR_VARIANT(accumulate_kernel, false, true, true),   HR_VARIANT(accumulate_kernel, true, true, true)};
// moments / sample_counts as the options have them; list: a tile mask is in force (it needs the counts: no <.., false, true> row)
static AccumulateFn select_accumulate_kernel(bool moments, bool counts, bool list) {
    return fn_of(find_row(ACCUMULATE_VARIANTS, [&](const AccumulateVariant &r) { return r.mom == moments && r.cnts == counts && r.list == list; }));
}

// ---- bucket_kernel<CNTS, LIST, BYS> (trace_kernel.h): a launch's per-sampling pixel values into the sample buckets (option robust_buckets) ----
typedef void (*BucketFn)(RenderParams, const float *, double *, const uint32_t *, uint32_t, unsigned long long);
// (a row of two flags is the ordinal form of option bucket_by_sampling 0: BYS takes its default, false)
struct BucketVariant {
    bool cnts, list, bys;
    BucketFn fn;
    constexpr BucketVariant(bool c, bool l, BucketFn f) : cnts(c), list(l), bys(false), fn(f) {}
    constexpr BucketVariant(bool c, bool l, bool b, BucketFn f) : cnts(c), list(l), bys(b), fn(f) {}
};
static const BucketVariant BUCKET_VARIANTS[] = {HR_VARIANT(bucket_kernel, false, false), HR_VARIANT(bucket_kernel, true, false), HR_VARIANT(bucket_kernel, true, true),
                                                // option bucket_by_sampling 1: the same three launches, the bucket taken from the sampling's index
                                                HR_VARIANT(bucket_kernel, false, false, true), HR_VARIANT(bucket_kernel, true, false, true), HR_VARIANT(bucket_kernel, true, true, true)};
// sample_counts / bucket_by_sampling as the options have them; list: a tile mask is in force (it needs the counts: no <false, true, ..> row)
static BucketFn select_bucket_kernel(bool counts, bool list, bool by_sampling) {
    return fn_of(find_row(BUCKET_VARIANTS, [&](const BucketVariant &r) { return r.cnts == counts && r.list == list && r.bys == by_sampling; }));
}

// ---- robust_noise_kernel<K, STAGE> (post_kernels.h): the robust noise estimate of the sample buckets, one row per K the option robust_buckets takes ----
// stage: the workgroup's span goes through LDS (what the library runs) — its rows want `lds` bytes of dynamic LDS (create_resources raises the limit:
// K = 11 and more is past 64 KiB); the per-lane form wants none and is kept for the comparison of DESIGN.md §4.11: a library built with
// -DHR_ROBUST_NOISE_PER_LANE (`make EXPFLAGS=-DHR_ROBUST_NOISE_PER_LANE`) runs it instead — the same bits, another time.
typedef void (*RobustNoiseFn)(const double *, const uint32_t *, unsigned long long, size_t, double, double, double *, uint8_t *, double *);
struct RobustNoiseVariant { uint32_t k; bool stage; RobustNoiseFn fn; uint32_t lds() const { return stage ? 256u * 3u * k * (uint32_t)sizeof(double) : 0u; } };
static const RobustNoiseVariant ROBUST_NOISE_VARIANTS[] = {
    HR_VARIANT(robust_noise_kernel, 3, true),   HR_VARIANT(robust_noise_kernel, 5, true),   HR_VARIANT(robust_noise_kernel, 7, true),  HR_VARIANT(robust_noise_kernel, 9, true),
    HR_VARIANT(robust_noise_kernel, 11, true),  HR_VARIANT(robust_noise_kernel, 13, true),  HR_VARIANT(robust_noise_kernel, 15, true),
    HR_VARIANT(robust_noise_kernel, 3, false),  HR_VARIANT(robust_noise_kernel, 5, false),  HR_VARIANT(robust_noise_kernel, 7, false), HR_VARIANT(robust_noise_kernel, 9, false),
    HR_VARIANT(robust_noise_kernel, 11, false), HR_VARIANT(robust_noise_kernel, 13, false), HR_VARIANT(robust_noise_kernel, 15, false),
};
#if defined(HR_ROBUST_NOISE_PER_LANE)
static const bool ROBUST_NOISE_STAGED = false;
#else
static const bool ROBUST_NOISE_STAGED = true;
#endif
// K as option robust_buckets has it; stage: ROBUST_NOISE_STAGED
static const RobustNoiseVariant *select_robust_noise_kernel(uint32_t k, bool stage) {
    return find_row(ROBUST_NOISE_VARIANTS, [&](const RobustNoiseVariant &r) { return r.k == k && r.stage == stage; });
}

// ---- robust_kernel<K> and robust_denoise_init_kernel<K> (post_kernels.h): hr_robust and the init pass of hr_denoise_robust, one row per K ----
// Both stage a workgroup's span through lds() bytes of dynamic LDS (robust_stage_span; create_resources raises the limit): a row of these
// families, and of restore_init_kernel's below, is a KRow of the kernel's type.
template <class Fn>
struct KRow { uint32_t k; Fn fn; uint32_t lds() const { return 256u * 3u * k * (uint32_t)sizeof(double); } };
typedef void (*RobustFn)(const double *, const uint32_t *, unsigned long long, float *, uint8_t *, size_t);
typedef KRow<RobustFn> RobustVariant;
static const RobustVariant ROBUST_VARIANTS[] = {
    HR_VARIANT(robust_kernel, 3),  HR_VARIANT(robust_kernel, 5),  HR_VARIANT(robust_kernel, 7),  HR_VARIANT(robust_kernel, 9),
    HR_VARIANT(robust_kernel, 11), HR_VARIANT(robust_kernel, 13), HR_VARIANT(robust_kernel, 15),
};
// K as option robust_buckets has it
static const RobustVariant *select_robust_kernel(uint32_t k) {
    return find_row(ROBUST_VARIANTS, [&](const RobustVariant &r) { return r.k == k; });
}
typedef void (*RobustDenoiseInitFn)(const double *, const uint32_t *, unsigned long long, const float *, double *, size_t, int);
typedef KRow<RobustDenoiseInitFn> RobustDenoiseInitVariant;
static const RobustDenoiseInitVariant ROBUST_DENOISE_INIT_VARIANTS[] = {
    HR_VARIANT(robust_denoise_init_kernel, 3),  HR_VARIANT(robust_denoise_init_kernel, 5),  HR_VARIANT(robust_denoise_init_kernel, 7),
    HR_VARIANT(robust_denoise_init_kernel, 9),  HR_VARIANT(robust_denoise_init_kernel, 11), HR_VARIANT(robust_denoise_init_kernel, 13),
    HR_VARIANT(robust_denoise_init_kernel, 15),
};
static const RobustDenoiseInitVariant *select_robust_denoise_init_kernel(uint32_t k) {
    return find_row(ROBUST_DENOISE_INIT_VARIANTS, [&](const RobustDenoiseInitVariant &r) { return r.k == k; });
}

// ---- restore_init_kernel<K> (post_kernels.h): the init pass of hr_robust_restore, {C, X} of every pixel, one row per K ----
// It stages a workgroup's span through lds() bytes of dynamic LDS as the two families above do (robust_stage_span; create_resources raises the limit).
typedef void (*RestoreInitFn)(const double *, const uint32_t *, unsigned long long, double *, size_t);
typedef KRow<RestoreInitFn> RestoreInitVariant;
static const RestoreInitVariant RESTORE_INIT_VARIANTS[] = {
    HR_VARIANT(restore_init_kernel, 3),  HR_VARIANT(restore_init_kernel, 5),  HR_VARIANT(restore_init_kernel, 7),  HR_VARIANT(restore_init_kernel, 9),
    HR_VARIANT(restore_init_kernel, 11), HR_VARIANT(restore_init_kernel, 13), HR_VARIANT(restore_init_kernel, 15),
};
// K as option robust_buckets has it
static const RestoreInitVariant *select_restore_init_kernel(uint32_t k) {
    return find_row(RESTORE_INIT_VARIANTS, [&](const RestoreInitVariant &r) { return r.k == k; });
}

// ---- select_init_kernel<K> (post_kernels.h): the init pass of hr_denoise_select, the three states and the halves' raw radiance, one row per K ----
// It stages a workgroup's span through lds() bytes of dynamic LDS as the three families above do (robust_stage_span; create_resources raises the limit).
typedef void (*SelectInitFn)(const double *, const uint32_t *, uint32_t, const float *, const double *, const float *, double *, double *, size_t, int);
typedef KRow<SelectInitFn> SelectInitVariant;
static const SelectInitVariant SELECT_INIT_VARIANTS[] = {
    HR_VARIANT(select_init_kernel, 3),  HR_VARIANT(select_init_kernel, 5),  HR_VARIANT(select_init_kernel, 7),  HR_VARIANT(select_init_kernel, 9),
    HR_VARIANT(select_init_kernel, 11), HR_VARIANT(select_init_kernel, 13), HR_VARIANT(select_init_kernel, 15),
};
// K as option robust_buckets has it
static const SelectInitVariant *select_select_init_kernel(uint32_t k) {
    return find_row(SELECT_INIT_VARIANTS, [&](const SelectInitVariant &r) { return r.k == k; });
}
