// hanamaru-hip — host driver with the reference binary's flag surface and outputs (main.rs:1226-1295,
// renderer.rs:205-251): `hanamaru-hip -w W -h H -s S -t SEC -i SEC`.  Stand-in for the Rust host (no Rust
// toolchain here): scene authoring + PNG writing stay on the host, the render loop calls the C ABI.
// Additive flags (do not change defaults): --scene NAME, --assets DIR, --batch N, --launch L, --inflight K, --precise, --gpus N / --gpu-ids LIST,
// --checkpoint FILE (write the fp32 accumulator + sampling count when the render stops) and --resume FILE
// (continue from such a file: samplings are independent and seeded by index, so a resumed render adds exactly
// the samplings that are missing — SURVEY.md §8f rank 3; the reference has no resumable state), --region X,Y,W,H (render the
// window [X, X+W) x [Y, Y+H) of the -w x -h frame, bit for bit the frame's pixels there: hr_set_region; the images are W x H),
// --noise-target E / --noise-floor F / --noise-check N / --noise-image FILE (option "moments": stop when the mean relative standard error of
// the pixels is <= E; hr_noise_estimate — the reference stops on a sampling count or the clock only),
// --adaptive E / --sample-image FILE (options "moments" + "sample_counts": after a uniform first phase only the 4x4 tiles that still hold a pixel
// with a relative standard error above E are rendered on; hr_select_tiles, hr_resolve_counted),
// --denoise / --denoise-levels N / --guide-image PREFIX (option "moments": the final image is the variance-guided a-trous filter's, hr_denoise +
// hr_resolve_denoised; the guide planes as images of their own, hr_render_guides + hr_read_guides), --guide-bounces K (option "guide_bounces":
// the guide rays follow mirrors and glass for up to K bounces to the first rough hit; 0, the default, is the first hit),
// --robust K / --robust-image FILE (option "robust_buckets": every image is the firefly-robust resolve of K sample buckets per pixel, hr_robust +
// hr_resolve_robust; the buckets ride in the checkpoint behind the other trailers).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hanamaru_hip.h"
#include "hanamaru_host.h"

static FILE *g_log = nullptr;
static void tee(const char *fmt, ...) {  // main.rs:47-51
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    printf("%s\n", buf);
    if (g_log) { fputs(buf, g_log); fputc('\n', g_log); }
}
static double now_sec() {
    using namespace std::chrono;
    return duration_cast<duration<double>>(steady_clock::now().time_since_epoch()).count();
}
#define CHECK_HR(expr)                                                          \
    do {                                                                        \
        int rc_ = (expr);                                                       \
        if (rc_ != 0) { fprintf(stderr, "%s: %s\n", #expr, hr_last_error()); return 1; } \
    } while (0)

static void usage(const char *prog) {
    printf("Usage: %s [options]\n\nOptions:\n"
           "        --help          print this help menu\n"
           "    -d, --debug         use debug mode\n"
           "    -w, --width WIDTH   output resolution width\n"
           "    -h, --height HEIGHT output resolution height\n"
           "    -s, --sampling SAMPLING\n                        sampling limit\n"
           "    -t, --time TIME     time limit sec\n"
           "    -i, --interval INTERVAL\n                        report interval sec\n"
           "        --scene NAME    rtcamp6_v3_1 (default) | rtcamp6_v3 | rtcamp6_v2 | rtcamp6_v1 | rtcamp5 | tbf3 | material_examples | simple |\n"
           "                        spheres | rtcamp6_dodeca | cornell_mini\n"
           "        --assets DIR    directory holding models/ and textures/ (default: ./assets, then .)\n"
           "        --batch N       samplings per progress report (default 1: one \"rendering:\" line per sampling, as the reference)\n"
           "        --launch L      reports per GPU launch (default 0: as many as fill the chip — 4 samplings per device at 1920x1080); the lines of a\n"
           "                        launch are printed when it is done, its time split evenly over them; 1 = a launch per report\n"
           "        --inflight K    launches enqueued ahead on the GPU (default 8; 1 = wait for every launch before the next starts)\n"
           "        --precise       precise shading: the geometry of every bounce in f64 from the reference's f64 draws (hr_set_option\n"
           "                        \"precise_shading\"): the reference's own arithmetic on refraction chains, small spheres and roughness maps;\n"
           "                        default: on for scenes without meshes (where it costs 2 - 4 %%), off for mesh scenes (7 - 30 %%);\n"
           "                        --no-precise: fp32 shading whatever the scene\n"
           "        --gpus N        render on devices 0..N-1 of this node from this one process: device r takes every N-th sampling,\n"
           "                        the accumulators are summed with one RCCL all-reduce when an image is written (default 1)\n"
           "        --gpu-ids LIST  the same with an explicit comma-separated device list\n"
           "        --checkpoint F  write accumulator + sampling count to F when the render stops\n"
           "        --resume F      continue from a checkpoint file\n"
           "        --region X,Y,W,H\n"
           "                        render only the window [X, X+W) x [Y, Y+H) of the -w x -h frame (border render): its pixels are the\n"
           "                        frame's, bit for bit, and the images are W x H; stitch tiles from their checkpoints' accumulators\n"
           "        --noise-target E\n"
           "                        keep per-pixel sample moments and stop as soon as the mean over the pixels of the relative standard error\n"
           "                        e = (se_r + se_g + se_b) / (r + g + b + 3 F) is <= E — or at -s samplings / the time limit, whichever comes\n"
           "                        first (0 = never reached: measure only).  Every check prints a line \"noise: samplings= mean= max= above=\"\n"
           "                        (above = pixels with e > E); the last one goes to result.txt as well\n"
           "        --noise-floor F radiance below which a pixel's error is judged absolutely instead of relatively (default 0.01; > 0)\n"
           "        --noise-check N ask every N samplings (default 64, rounded up to whole launches): the question waits for the launches\n"
           "                        in flight, so it is asked rarely\n"
           "        --adaptive E    adaptive sampling: render uniformly until the first check (--noise-check, default 64 samplings), then at every\n"
           "                        check keep only the 4x4-pixel tiles that hold a pixel whose relative standard error e is above E, and stop\n"
           "                        when no tile is left, or at -s / -t, whichever comes first.  Every check prints a line \"adaptive: samplings=\n"
           "                        active= tiles=\".  The images are resolved with every pixel's own sampling count.  Choosing the tiles by the\n"
           "                        samples that form the estimate biases the image slightly; the uniform first phase keeps that small.\n"
           "                        One device only; not together with --noise-target (two stop rules).\n"
           "        --sample-image FILE.png\n"
           "                        write the per-pixel sampling counts as 8-bit grey, count / largest count (one device only)\n"
           "        --noise-image FILE.png\n"
           "                        write an 8-bit grey map of min(1, e / E) at the end of the render (E = the target, or 0.05 without one)\n"
           "        --denoise       keep per-pixel sample moments and write the FINAL image through the variance-guided edge-avoiding a-trous filter\n"
           "                        (hr_denoise: guided by first-hit albedo, normal and depth; progress images stay as they are).  With --adaptive\n"
           "                        every pixel's own sampling count is its n.  One device only; not with --debug.\n"
           "        --denoise-levels N\n"
           "                        filter levels, 0 .. 5 (default 4; the taps of level l are 2^l pixels apart)\n"
           "        --guide-image PREFIX\n"
           "                        write the guide planes as PREFIX_albedo.png, PREFIX_normal.png ((n + 1) / 2) and PREFIX_depth.png (depth / largest\n"
           "                        depth, grey).  One device only; not with --debug.\n"
           "        --guide-bounces K\n"
           "                        the guide planes follow mirrors and glass (Specular and Refraction surfaces) for up to K bounces, 0 .. 8, to the\n"
           "                        first rough hit: albedo is the product along the chain, the normal the last hit's, depth the path length.\n"
           "                        Default 0: the first hit.  Needs --denoise or --guide-image.\n"
           "        --robust K      keep K sample buckets per pixel (K odd, 3 .. 15; 3 K doubles per pixel) and write every image, progress and final,\n"
           "                        through the firefly-robust resolve (hr_robust + hr_resolve_robust: an adaptive median of the K bucket means, which\n"
           "                        drops the buckets a few very bright paths landed in; biased dark where it trims).  Works with --region,\n"
           "                        --noise-target and --adaptive (every pixel's own sampling count).  --checkpoint appends the buckets, --resume\n"
           "                        restores them and refuses a file without them or with another K.  One device only; not with --denoise or --debug.\n"
           "        --robust-image FILE.png\n"
           "                        write an 8-bit grey map of trim / ((K - 1) / 2), the buckets dropped at either end (needs --robust)\n",
           prog);
}

int main(int argc, char **argv) {
    uint32_t width = 1920, height = 1080, sampling = 1000;  // main.rs:1249-1251
    double time_limit = 123.0, interval = 15.0;              // main.rs:1255-1256
    std::string scene_name = "rtcamp6_v3_1", assets, ckpt_out, ckpt_in, gpu_ids;
    int gpus = 1;
    int batch = 1;      // samplings per report_progress call ("rendering:" line); 1 = the reference's cadence
    int launch = 0;     // reports per GPU launch; 0 = as many as fill the chip (4 samplings per device at 1920x1080)
    int inflight = 8;   // launches enqueued ahead of the one being reported
    bool debug = false;
    int precise = -1;    // option precise_shading: -1 = the library's automatic choice
    std::string region_arg, noise_png, sample_png;
    bool have_adaptive = false;
    double adaptive_e = 0.0;
    bool have_target = false;
    double noise_target = 0.0, noise_floor = 0.01;
    long long noise_check = 64;
    bool denoise = false;
    long long denoise_levels = -1;   // -1: the library's default
    std::string guide_prefix;
    long long guide_bounces = -1;    // -1: not given (the library's default, 0)
    long long robust_k = 0;          // --robust K: option "robust_buckets" (0: off)
    std::string robust_png;
    // a number, the whole argument, not NaN; what is wrong with it is said with the flag's name, before any device is opened
    auto number = [](const char *flag, const char *text, double *out) -> bool {
        char *e = nullptr;
        *out = strtod(text, &e);
        if (e == text || *e || std::isnan(*out) || std::isinf(*out)) { fprintf(stderr, "%s: '%s' is not a number.\n", flag, text); return false; }
        return true;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "Argument to option '%s' missing.\n", name); exit(1); }
            return argv[++i];
        };
        if (a == "--help") { usage(argv[0]); return 0; }
        else if (a == "-d" || a == "--debug") debug = true;
        else if (a == "-w" || a == "--width") width = (uint32_t)strtoul(val("w"), nullptr, 10);
        else if (a == "-h" || a == "--height") height = (uint32_t)strtoul(val("h"), nullptr, 10);
        else if (a == "-s" || a == "--sampling") sampling = (uint32_t)strtoul(val("s"), nullptr, 10);
        else if (a == "-t" || a == "--time") time_limit = strtod(val("t"), nullptr);
        else if (a == "-i" || a == "--interval") interval = strtod(val("i"), nullptr);
        else if (a == "--scene") scene_name = val("scene");
        else if (a == "--assets") assets = val("assets");
        else if (a == "--batch") batch = atoi(val("batch"));
        else if (a == "--launch") launch = atoi(val("launch"));
        else if (a == "--inflight") inflight = atoi(val("inflight"));
        else if (a == "--precise") precise = 1;
        else if (a == "--no-precise") precise = 0;
        else if (a == "--gpus") gpus = atoi(val("gpus"));
        else if (a == "--gpu-ids") gpu_ids = val("gpu-ids");
        else if (a == "--checkpoint") ckpt_out = val("checkpoint");
        else if (a == "--resume") ckpt_in = val("resume");
        else if (a == "--region") region_arg = val("region");
        else if (a == "--noise-target") {
            if (!number("--noise-target", val("noise-target"), &noise_target)) return 1;
            if (noise_target < 0.0) { fprintf(stderr, "--noise-target must not be negative.\n"); return 1; }
            have_target = true;
        } else if (a == "--noise-floor") {
            if (!number("--noise-floor", val("noise-floor"), &noise_floor)) return 1;
            if (!(noise_floor > 0.0)) { fprintf(stderr, "--noise-floor must be positive.\n"); return 1; }
        } else if (a == "--noise-check") {
            const char *t = val("noise-check");
            char *e = nullptr;
            noise_check = strtoll(t, &e, 10);
            if (e == t || *e || noise_check < 1 || noise_check > 0x7fffffffll) { fprintf(stderr, "--noise-check must be a whole number of samplings, at least 1, not '%s'.\n", t); return 1; }
        } else if (a == "--noise-image") noise_png = val("noise-image");
        else if (a == "--adaptive") {
            if (!number("--adaptive", val("adaptive"), &adaptive_e)) return 1;
            if (!(adaptive_e > 0.0)) { fprintf(stderr, "--adaptive must be positive.\n"); return 1; }
            have_adaptive = true;
        } else if (a == "--sample-image") sample_png = val("sample-image");
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-levels") {
            const char *t = val("denoise-levels");
            char *e = nullptr;
            denoise_levels = strtoll(t, &e, 10);
            if (e == t || *e || denoise_levels < 0 || denoise_levels > 5) { fprintf(stderr, "--denoise-levels must be a whole number in 0 .. 5, not '%s'.\n", t); return 1; }
        } else if (a == "--guide-image") guide_prefix = val("guide-image");
        else if (a == "--guide-bounces") {
            const char *t = val("guide-bounces");
            char *e = nullptr;
            guide_bounces = strtoll(t, &e, 10);
            if (e == t || *e || guide_bounces < 0 || guide_bounces > 8) { fprintf(stderr, "--guide-bounces must be a whole number in 0 .. 8, not '%s'.\n", t); return 1; }
        }
        else if (a == "--robust") {
            const char *t = val("robust");
            char *e = nullptr;
            robust_k = strtoll(t, &e, 10);
            if (e == t || *e || robust_k < 3 || robust_k > 15 || !(robust_k & 1)) { fprintf(stderr, "--robust must be an odd number of buckets in 3 .. 15, not '%s'.\n", t); return 1; }
        } else if (a == "--robust-image") robust_png = val("robust-image");
        else { fprintf(stderr, "Unrecognized option: '%s'.\n", a.c_str()); return 1; }
    }
    if (batch < 1) { fprintf(stderr, "--batch must be at least 1.\n"); return 1; }
    if (launch < 0) { fprintf(stderr, "--launch must be at least 1 (or 0: automatic).\n"); return 1; }
    if (inflight < 1) { fprintf(stderr, "--inflight must be at least 1.\n"); return 1; }
    if (width == 0 || height == 0) { fprintf(stderr, "width and height must be positive.\n"); return 1; }
    if (gpus < 1) { fprintf(stderr, "--gpus must be at least 1.\n"); return 1; }
    const bool counts = have_adaptive || !sample_png.empty();   // hr_set_option "sample_counts"
    if (counts) {
        size_t ids = gpu_ids.empty() ? 0 : 1;
        for (char ch : gpu_ids) ids += ch == ',';
        if (gpus > 1 || ids > 1) {
            fprintf(stderr, "--adaptive / --sample-image render on one device: the library can shard an adaptive render (masks and additive counts), this program's device loop does not.\n");
            return 1;
        }
        if (have_adaptive && have_target) { fprintf(stderr, "--adaptive and --noise-target are two stop rules: give one of them.\n"); return 1; }
        if (debug) { fprintf(stderr, "--adaptive / --sample-image cannot be combined with --debug (the debug renderer has no samplings to count).\n"); return 1; }
    }
    if (denoise_levels >= 0 && !denoise) { fprintf(stderr, "--denoise-levels needs --denoise.\n"); return 1; }
    if (guide_bounces >= 0 && !denoise && guide_prefix.empty()) { fprintf(stderr, "--guide-bounces needs --denoise or --guide-image.\n"); return 1; }
    if (denoise || !guide_prefix.empty()) {
        size_t ids = gpu_ids.empty() ? 0 : 1;
        for (char ch : gpu_ids) ids += ch == ',';
        if (gpus > 1 || ids > 1) {
            fprintf(stderr, "--denoise / --guide-image render on one device: the library denoises one context's accumulator, moments and counts (a sharded host sums them into one), this program's device loop does not.\n");
            return 1;
        }
        if (debug) { fprintf(stderr, "--denoise / --guide-image cannot be combined with --debug (the debug renderer has no samplings whose variance could guide a filter).\n"); return 1; }
    }
    if (!robust_png.empty() && !robust_k) { fprintf(stderr, "--robust-image needs --robust.\n"); return 1; }
    if (robust_k) {
        size_t ids = gpu_ids.empty() ? 0 : 1;
        for (char ch : gpu_ids) ids += ch == ',';
        if (gpus > 1 || ids > 1) {
            fprintf(stderr, "--robust renders on one device: buckets of several devices add up only when each rendered a multiple of K samplings, and this program's device loop does not see to that.\n");
            return 1;
        }
        if (denoise) { fprintf(stderr, "--robust cannot be combined with --denoise (the filter reads the raw moments, not the robust radiance: two final images).\n"); return 1; }
        if (debug) { fprintf(stderr, "--robust cannot be combined with --debug (the debug renderer has no samplings to put into buckets).\n"); return 1; }
    }
    const bool moments = have_target || !noise_png.empty() || have_adaptive || denoise;   // hr_set_option "moments"
    if (moments && debug) { fprintf(stderr, "--noise-target / --noise-image cannot be combined with --debug (the debug renderer has no samplings to measure).\n"); return 1; }
    const double noise_e = have_adaptive ? adaptive_e : have_target && noise_target > 0.0 ? noise_target : (have_target ? 0.0 : 0.05);   // the threshold of "above" and of the grey map
    // --region X,Y,W,H: four unsigned integers, a non-empty window inside the frame (hr_set_region's rule, checked before any device is opened)
    uint32_t region[4] = {0, 0, width, height};
    bool has_region = false;
    if (!region_arg.empty()) {
        uint64_t v[4];
        int n = 0;
        for (const char *p = region_arg.c_str(); n < 4; n++) {
            if (*p < '0' || *p > '9') break;
            char *e = nullptr;
            v[n] = strtoull(p, &e, 10);
            if (v[n] > 0xffffffffull) break;
            p = e;
            if (n < 3 && *p++ != ',') break;
            if (n == 3 && *p) break;
        }
        if (n != 4) { fprintf(stderr, "--region must be X,Y,W,H (four unsigned integers), not '%s'.\n", region_arg.c_str()); return 1; }
        if (!v[2] || !v[3] || v[0] > width || v[2] > width - v[0] || v[1] > height || v[3] > height - v[1]) {
            fprintf(stderr, "--region %s: the window must be non-empty and lie inside the %ux%u frame.\n", region_arg.c_str(), width, height);
            return 1;
        }
        for (int k = 0; k < 4; k++) region[k] = (uint32_t)v[k];
        has_region = region[2] != width || region[3] != height;   // the whole frame as a region is no region
    }
    const uint32_t out_w = region[2], out_h = region[3];   // the accumulator and the images: the region's
    if (assets.empty()) {
        FILE *probe = fopen("assets/models/box.obj", "rb");
        if (probe) { fclose(probe); assets = "assets"; } else assets = ".";
    }
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);   // dmabuf IPC (RCCL on this driver), unless the caller says otherwise; before the HIP runtime starts
    g_log = fopen("result.txt", "w");
    double total_begin = now_sec();
    tee("num threads: %d.", 1);  // main.rs:1261 prints rayon's pool size; here: one host thread drives one GPU
    tee("resolution: %ux%u.", width, height);
    if (has_region) tee("region: %u,%u %ux%u.", region[0], region[1], out_w, out_h);
    tee("max sampling: %ux%u spp.", sampling, 4u);
    tee("time limit: %.2f sec.", time_limit);
    tee("report interval: %.2f sec.", interval);

    double init_begin = now_sec();
    hh_scene *scene = nullptr;
    if (hh_scene_create(scene_name.c_str(), assets.c_str(), &scene) != 0) { fprintf(stderr, "scene: %s\n", hh_last_error()); return 1; }
    // devices: samplings are independent and seeded by index, so device r of N renders samplings first + r, first + r + N, ...
    // (bench.py does the same with one process per GPU and an RCCL all-reduce)
    std::vector<int> devices;
    if (!gpu_ids.empty()) {
        for (size_t p = 0; p < gpu_ids.size();) {
            size_t q = gpu_ids.find(',', p);
            devices.push_back(atoi(gpu_ids.substr(p, q == std::string::npos ? std::string::npos : q - p).c_str()));
            if (q == std::string::npos) break;
            p = q + 1;
        }
    } else {
        for (int d = 0; d < (gpus > 0 ? gpus : 1); d++) devices.push_back(d);
    }
    const uint32_t ndev = (uint32_t)devices.size();
    std::vector<hr_ctx *> ctxs(ndev, nullptr);
    for (uint32_t r = 0; r < ndev; r++) {
        CHECK_HR(hr_create(devices[r], &ctxs[r]));
        CHECK_HR(hr_upload_scene(ctxs[r], hh_scene_desc(scene)));
        CHECK_HR(hr_set_resolution(ctxs[r], width, height));
        if (has_region) CHECK_HR(hr_set_region(ctxs[r], region[0], region[1], out_w, out_h));
        if (precise >= 0) CHECK_HR(hr_set_option(ctxs[r], "precise_shading", (double)precise));
        if (moments) CHECK_HR(hr_set_option(ctxs[r], "moments", 1.0));
        if (counts) CHECK_HR(hr_set_option(ctxs[r], "sample_counts", 1.0));
        if (guide_bounces >= 0) CHECK_HR(hr_set_option(ctxs[r], "guide_bounces", (double)guide_bounces));
        if (robust_k) CHECK_HR(hr_set_option(ctxs[r], "robust_buckets", (double)robust_k));
    }
    hr_ctx *ctx = ctxs[0];
    if (ndev > 1) tee("devices: %u.", ndev);
    tee("init scene: %.2f sec.", now_sec() - init_begin);
    // The image needs the sum of all devices' accumulators: ONE all-reduce over RCCL (hr_allreduce_accumulators — the sum lands
    // in a separate buffer per device, so every device keeps accumulating its own samplings afterwards); hr_resolve /
    // hr_read_accumulator on device 0 then see the total (renderer.rs:64-90 runs after the sum).
    // A multi-GPU box whose RCCL cannot be loaded (hr_comm_init_local: HR_ERR_UNSUPPORTED) still renders: the host then sums the
    // devices' accumulators itself when an image or a checkpoint is written (`sum_acc` below) — slower, same result.
    bool host_sum = false;
    if (ndev > 1) {
        int rc = hr_comm_init_local(ctxs.data(), (int)ndev);
        if (rc == HR_ERR_UNSUPPORTED) { host_sum = true; tee("no RCCL (%s): accumulators are summed on the host.", hr_last_error()); }
        else if (rc != 0) { fprintf(stderr, "hr_comm_init_local: %s\n", hr_last_error()); return 1; }
    }
    std::vector<float> sum_acc, part;
    auto combine = [&]() -> int {
        if (ndev == 1) return 0;
        if (!host_sum) return hr_allreduce_accumulators(ctxs.data(), (int)ndev) != 0;
        sum_acc.resize((size_t)out_w * out_h * 3);
        part.resize(sum_acc.size());
        if (hr_read_accumulator(ctxs[0], sum_acc.data()) != 0) return 1;
        for (uint32_t r = 1; r < ndev; r++) {
            if (hr_read_accumulator(ctxs[r], part.data()) != 0) return 1;
            for (size_t i = 0; i < sum_acc.size(); i++) sum_acc[i] += part[i];
        }
        return 0;
    };
    // host-side sum: device 0 resolves the total from its accumulator, then gets its own partial sums back
    bool have_guides = false;   // the context holds guide planes (for --guide-image)
    bool final_image = false;   // set by whoever writes the render's last image: --denoise filters that one only
    auto resolve = [&](uint32_t s, uint8_t *out) -> int {
        if (robust_k) return hr_robust(ctx) != 0 ? 1 : hr_resolve_robust(ctx, out);   // (one device, no --denoise: checked with the flags)
        if (denoise && final_image) {
            hr_denoise_params dp;
            if (hr_denoise_default_params(&dp) != 0) return 1;
            if (denoise_levels >= 0) dp.levels = (uint32_t)denoise_levels;
            const int rc = hr_denoise(ctx, &dp);   // (HR_ERR_INVALID: a pixel with fewer than 2 samplings — the flags' values were checked when they were read)
            if (rc == 0) { have_guides = true; return hr_resolve_denoised(ctx, out); }   // (hr_denoise rendered the guide planes, nothing has dropped them since)
            if (rc != HR_ERR_INVALID) return rc;
            tee("denoise: fewer than 2 samplings behind a pixel, the image is not denoised.");
        }
        if (have_adaptive) return hr_resolve_counted(ctx, out);   // every pixel with its own count (one device: checked with the flags)
        if (!host_sum) return hr_resolve(ctx, s, out);
        if (hr_read_accumulator(ctx, part.data()) != 0 || hr_write_accumulator(ctx, sum_acc.data()) != 0) return 1;
        int rc = hr_resolve(ctx, s, out);
        return hr_write_accumulator(ctx, part.data()) != 0 ? 1 : rc;
    };

    // The noise estimate of everything rendered so far.  Several devices: every device holds the moments of its own samplings; they are
    // additive, so the host adds them in rank order (as sum_acc does for accumulators without RCCL), device 0 estimates the total and gets
    // its own moments back.  tot_out / n_out: the summed moments and their count as well (for the checkpoint).
    // Returns 0, 1 = error, 2 = fewer than two samplings behind the moments (no variance yet).
    std::vector<double> mom_tot, mom_part, mom_own;
    auto noise_query = [&](hr_noise *est, double *img, std::vector<double> *tot_out, uint64_t *n_out) -> int {
        uint64_t n_own = 0, n_tot = 0;
        const size_t len = (size_t)out_w * out_h * 6;
        if (ndev > 1 || tot_out) {
            mom_tot.resize(len);
            if (hr_read_moments(ctx, mom_tot.data(), &n_own) != 0) return 1;
            n_tot = n_own;
        }
        if (ndev > 1) {
            mom_own = mom_tot;
            mom_part.resize(len);
            for (uint32_t r = 1; r < ndev; r++) {
                uint64_t n_r = 0;
                if (hr_read_moments(ctxs[r], mom_part.data(), &n_r) != 0) return 1;
                for (size_t i = 0; i < len; i++) mom_tot[i] += mom_part[i];
                n_tot += n_r;
            }
            if (hr_write_moments(ctx, mom_tot.data(), n_tot) != 0) return 1;
        }
        memset(est, 0, sizeof *est);
        int rc = hr_noise_estimate(ctx, noise_floor, noise_e, est);   // (HR_ERR_INVALID: n < 2 — floor and threshold were checked with the flags)
        if (rc == 0 && img) rc = hr_read_noise_image(ctx, noise_floor, img);
        if (ndev > 1 && hr_write_moments(ctx, mom_own.data(), n_own) != 0) return 1;
        if (tot_out) *tot_out = mom_tot;
        if (n_out) *n_out = n_tot;
        return rc == 0 ? 0 : (rc == HR_ERR_INVALID ? 2 : 1);
    };
    hr_noise noise_last;
    bool noise_known = false;
    // one "noise:" line per check, after the "rendering:" lines of the samplings it covers
    auto noise_check_now = [&]() -> int {
        int rc = noise_query(&noise_last, nullptr, nullptr, nullptr);
        if (rc == 1) { fprintf(stderr, "hr_noise_estimate: %s\n", hr_last_error()); return 1; }
        noise_known = rc == 0;
        if (noise_known) printf("noise: samplings=%llu mean=%.9g max=%.9g above=%llu\n", (unsigned long long)noise_last.samplings, noise_last.mean_error, noise_last.max_error,
                                (unsigned long long)noise_last.pixels_above);
        return 0;
    };
    std::vector<uint8_t> rgb((size_t)out_w * out_h * 3);
    double begin = now_sec(), last_progress = begin, last_image = begin;
    uint32_t counter = 0, sampled = 0;
    std::string last_png;     // the image file save() wrote last: result.png is a copy of the final one (one PNG encode, not two)
    auto save = [&](uint32_t s) -> int {
        char path[32];
        snprintf(path, sizeof path, "%03u.png", counter);
        double t0 = now_sec();
        if (combine() || resolve(s, rgb.data()) != 0) { fprintf(stderr, "hr_resolve: %s\n", hr_last_error()); return 1; }
        printf("update_imgbuf: %.3f sec\n", now_sec() - t0);
        last_png = path;
        return hh_write_png_rgb8(path, rgb.data(), out_w, out_h);
    };
    uint32_t first = 1;
    // checkpoint = {magic, width, height, samplings done, FNV-1a of the scene name} + the fp32 accumulator; with a region the magic is
    // "HRR2" and the header goes on with {x0, y0, w, h}, the accumulator is the region's (a full-frame checkpoint keeps the "HRA2" format)
    const uint32_t CKPT_MAGIC = 0x32415248u;          // "HRA2"
    const uint32_t CKPT_REGION_MAGIC = 0x32525248u;   // "HRR2"
    const uint32_t CKPT_MOMENTS_MAGIC = 0x534d5248u;  // "HRMS": the trailer behind the accumulator of a render with moments on
    const uint32_t CKPT_COUNTS_MAGIC = 0x43535248u;   // "HRSC": the trailer behind that of a render with sample counts on — w*h uint32
    const uint32_t CKPT_BUCKETS_MAGIC = 0x4b425248u;  // "HRBK": the trailer behind those of a render with --robust — K (uint32), samplings (uint64), w*h*3K doubles
    bool resumed_counts = false;                      // --resume restored per-pixel counts: the tiles are chosen again before anything is rendered
    uint32_t scene_hash = 2166136261u;
    for (char ch : scene_name) scene_hash = (scene_hash ^ (uint8_t)ch) * 16777619u;
    if (!ckpt_in.empty()) {
        FILE *f = fopen(ckpt_in.c_str(), "rb");
        uint32_t hdr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<float> acc((size_t)out_w * out_h * 3);
        bool ok = f && fread(hdr, 4, 5, f) == 5 && (hdr[0] == CKPT_MAGIC || hdr[0] == CKPT_REGION_MAGIC);
        if (ok && (hdr[0] == CKPT_REGION_MAGIC) != has_region) {
            if (f) fclose(f);
            fprintf(stderr, "cannot resume from %s: %s\n", ckpt_in.c_str(), has_region ? "it is a full-frame checkpoint and --region is given" : "it is a region checkpoint and no --region is given");
            return 1;
        }
        if (ok && has_region) {
            ok = fread(hdr + 5, 4, 4, f) == 4;
            if (ok && (hdr[5] != region[0] || hdr[6] != region[1] || hdr[7] != out_w || hdr[8] != out_h)) {
                fclose(f);
                fprintf(stderr, "cannot resume from %s: its region is %u,%u,%u,%u, --region is %u,%u,%u,%u\n", ckpt_in.c_str(), hdr[5], hdr[6], hdr[7], hdr[8],
                        region[0], region[1], out_w, out_h);
                return 1;
            }
        }
        ok = ok && hdr[1] == width && hdr[2] == height && hdr[4] == scene_hash && fread(acc.data(), sizeof(float), acc.size(), f) == acc.size();
        // a checkpoint written with moments on goes on with the trailer {"HRMS", samplings behind the moments, w*h*6 doubles}
        uint32_t mmagic = 0;
        uint64_t mom_n = 0;
        std::vector<double> mom;
        bool have_mom = false;
        std::vector<uint32_t> cnt;
        if (ok && (moments || counts || robust_k) && fread(&mmagic, 4, 1, f) == 1 && mmagic == CKPT_MOMENTS_MAGIC) {
            mom.resize((size_t)out_w * out_h * 6);
            have_mom = fread(&mom_n, 8, 1, f) == 1 && fread(mom.data(), sizeof(double), mom.size(), f) == mom.size();
            if (have_mom && fread(&mmagic, 4, 1, f) != 1) mmagic = 0;   // what follows the moments
            have_mom = have_mom && moments;
        }
        if (ok && counts) {
            // {"HRSC", w*h uint32}; a file without it was rendered uniformly: every pixel has received all of its samplings
            cnt.assign((size_t)out_w * out_h, hdr[3]);
            if (mmagic == CKPT_COUNTS_MAGIC) {
                resumed_counts = fread(cnt.data(), sizeof(uint32_t), cnt.size(), f) == cnt.size();
                ok = resumed_counts;
                if (ok && fread(&mmagic, 4, 1, f) != 1) mmagic = 0;   // what follows the counts
            }
        }
        // {"HRBK", K, samplings behind the buckets, w*h*3K doubles}
        std::vector<double> bkt;
        uint32_t bkt_k = 0;
        uint64_t bkt_n = 0;
        const char *bkt_why = nullptr;
        if (ok && robust_k) {
            if (!counts && mmagic == CKPT_COUNTS_MAGIC) bkt_why = "its buckets were filled by per-pixel sampling counts (resume with --adaptive or --sample-image as well)";
            else if (mmagic != CKPT_BUCKETS_MAGIC || fread(&bkt_k, 4, 1, f) != 1 || fread(&bkt_n, 8, 1, f) != 1) bkt_why = "it holds no sample buckets (it was written without --robust)";
            else if (bkt_k != (uint32_t)robust_k) bkt_why = "its sample buckets were kept with another K";
            else {
                bkt.resize((size_t)out_w * out_h * 3 * bkt_k);
                ok = fread(bkt.data(), sizeof(double), bkt.size(), f) == bkt.size();
            }
        }
        if (f) fclose(f);
        if (!ok) { fprintf(stderr, "cannot resume from %s (missing, wrong magic, resolution or scene)\n", ckpt_in.c_str()); return 1; }
        if (bkt_why) {
            fprintf(stderr, "--resume %s with --robust %lld: %s; resume without --robust, or render again with it.\n", ckpt_in.c_str(), robust_k, bkt_why);
            return 1;
        }
        if (have_adaptive && !have_mom) {
            fprintf(stderr, "--resume %s with --adaptive: the checkpoint holds no sample moments (it was written without --adaptive / --noise-target / --noise-image), "
                            "so the noise of its %u samplings cannot be known; resume without --adaptive, or render again with it.\n", ckpt_in.c_str(), hdr[3]);
            return 1;
        }
        if (have_adaptive && !resumed_counts && mom_n != hdr[3]) {
            fprintf(stderr, "--resume %s with --adaptive: its sample moments cover %llu of its %u samplings and it holds no per-pixel counts, "
                            "so the noise of its pixels cannot be known; resume without --adaptive, or render again with it.\n", ckpt_in.c_str(), (unsigned long long)mom_n, hdr[3]);
            return 1;
        }
        if (denoise && !(have_mom && (resumed_counts || mom_n == hdr[3]))) {
            // the filter's mean is accumulator / (4 n) with n the samplings behind the moments (or the pixel's count): moments that do not cover
            // every sampling of the accumulator would give an image of the wrong brightness
            fprintf(stderr, "--resume %s with --denoise: the checkpoint's sample moments %s, so the variance of its %u samplings cannot be known; "
                            "resume without --denoise, or render again with it.\n", ckpt_in.c_str(),
                    have_mom ? "do not cover all of its samplings" : "are missing (it was written without --denoise / --adaptive / --noise-target / --noise-image)", hdr[3]);
            return 1;
        }
        if (have_target && !have_mom) {
            fprintf(stderr, "--resume %s with --noise-target: the checkpoint holds no sample moments (it was written without --noise-target / --noise-image), "
                            "so the noise of its %u samplings cannot be known; resume without --noise-target, or render again with it.\n", ckpt_in.c_str(), hdr[3]);
            return 1;
        }
        CHECK_HR(hr_write_accumulator(ctx, acc.data()));
        if (counts) CHECK_HR(hr_write_sample_counts(ctx, cnt.data()));
        if (have_mom) CHECK_HR(hr_write_moments(ctx, mom.data(), mom_n));
        else if (moments) printf("the checkpoint holds no sample moments: the noise image covers the samplings rendered from here on\n");
        if (robust_k) CHECK_HR(hr_write_buckets(ctx, bkt.data(), bkt_n));
        first = hdr[3] + 1;
        sampled = hdr[3];
        printf("resumed at %ux4 sampled\n", hdr[3]);
    }
    if (debug) {  // main.rs:1279-1281: DebugRenderer { mode: FocalPlane }, max_sampling 1, report_progress = update_imgbuf + stop
        CHECK_HR(hr_render_debug(ctx, 3));
        CHECK_HR(hr_synchronize(ctx));
        CHECK_HR(hr_resolve(ctx, 1, rgb.data()));
        sampled = 1;
        sampling = 0;
    }
    // Renderer::render's loop with report_progress (renderer.rs:32-43, 205-251).  What is REPORTED and what is LAUNCHED are two things:
    //   * a REPORT = `--batch` samplings = one "rendering:" line; the default, --batch 1, is the reference's own cadence: a line per sampling;
    //   * the GPU is fed LAUNCHES of whole reports — `--launch` of them, by default as many as fill the chip (4 samplings per device at
    //     1920x1080: one kernel launch per sampling costs 3 - 8 % of the rate) — and up to --inflight launches are enqueued ahead
    //     (hr_render only enqueues; hr_mark behind every launch, hr_wait for the oldest), so the GPU never drains between progress lines.
    //     When a launch is done its reports are printed together: the launch's wall time is split EVENLY over their lines (said once in the log).
    // report_progress's three rules keep their order and their meaning:
    //   * time limit (renderer.rs:222-231: stop when used + 1.1 x last > limit, `last` = seconds per report).  The reference asks this after
    //     a sampling, before it starts the next; here the question is asked when reports are ISSUED, for the moment they would finish: n
    //     reports are issued only if used + 1.1 x last x (reports in flight + n) <= limit, and a launch shrinks to the n that still fits
    //     (down to one report).  With one report in flight at a time (-i 0, or --launch 1 --inflight 1) that is the reference's rule to the
    //     letter.  When everything in flight has been reported and nothing may follow, the final image is written: "reached time limit"
    //     if the rule says so, else "reached max sampling" (in that order, renderer.rs:222-241).
    //   * progress image (renderer.rs:243-251): asked at launch boundaries (the accumulator holds whole launches); when the interval has
    //     passed, the launches in flight are awaited and reported first, so that the image holds exactly the samplings of the
    //     "rendering:" line before it, as in the reference (one pipeline drain per image).  An interval of 0 asks for an image after
    //     every report: launches are then one report long, one in flight, and `-s 5 -i 0` prints and writes exactly what the
    //     reference does — 000.png .. 003.png after samplings 1 .. 4, final 004.png.
    struct Launch { uint32_t begin, end; double issued; std::vector<uint64_t> ticket; };
    std::vector<Launch> q;     // issued, not yet reported; oldest first
    uint32_t next_s = first;
    const uint32_t B = (uint32_t)batch;
    uint32_t lrep = launch > 0 ? (uint32_t)launch : 0;   // reports per launch
    if (!lrep) {   // as many reports as make the library's own automatic launch size (hanamaru_hip.h "batch": about 33 M paths) on every device
        const uint64_t per_sampling = ((uint64_t)(out_w + 3) / 4) * ((out_h + 3) / 4) * 64u;
        const uint64_t lsize = std::min<uint64_t>(64, std::max<uint64_t>(4, (33177600ull + per_sampling - 1) / per_sampling));
        lrep = (uint32_t)std::max<uint64_t>(1, lsize * ndev / B);
    }
    if (interval <= 0.0) lrep = 1;
    if (lrep > 1 && !debug) printf("launches of %u reports (%u samplings): a launch's time is split evenly over its reports' lines.\n", lrep, lrep * B);
    uint32_t in_flight = 0;   // reports issued, not yet printed
    auto reports_of = [&](uint32_t b, uint32_t e) { return (e - b + B - 1) / B; };
    auto issue = [&](uint32_t nrep) -> int {
        Launch c;
        c.begin = next_s;
        c.end = (uint64_t)next_s + (uint64_t)nrep * B > (uint64_t)sampling + 1 ? sampling + 1 : next_s + nrep * B;
        c.issued = now_sec();
        c.ticket.assign(ndev, 0);
        for (uint32_t r = 0; r < ndev; r++) {
            // device r of N renders the samplings with (s - 1) mod N == r, whatever the launch's first sampling is — a launch
            // shorter than N leaves some devices without work, their marker is then reached at once
            const uint32_t b = c.begin + (r + ndev - (c.begin - 1u) % ndev) % ndev;
            if (hr_render(ctxs[r], b, c.end, ndev) != 0 || hr_mark(ctxs[r], &c.ticket[r]) != 0) { fprintf(stderr, "hr_render: %s\n", hr_last_error()); return 1; }
        }
        next_s = c.end;
        in_flight += reports_of(c.begin, c.end);
        q.push_back(c);
        return 0;
    };
    bool measured = false;    // has any launch been reported?  (a measured zero is a measurement)
    double last = 0.0;        // `from_last_sampling_sec`: seconds per report of the last launch reported
    double used = 0.0;
    // wait for the oldest launch in flight and print its reports' lines (renderer.rs:206-214)
    auto report = [&]() -> int {
        const Launch c = q.front();
        q.erase(q.begin());
        for (uint32_t r = 0; r < ndev; r++)
            if (hr_wait(ctxs[r], c.ticket[r]) != 0) { fprintf(stderr, "hr_wait: %s\n", hr_last_error()); return 1; }
        const double now = now_sec();
        const uint32_t n = reports_of(c.begin, c.end);
        // the launch's own time: from the previous report (the pipeline is full: launches finish back to back), or from its issue if that is later
        const double t0 = std::max(last_progress, c.issued);
        last = (now - t0) / (double)n;
        measured = true;
        for (uint32_t j = 0; j < n; j++) {
            sampled = std::min(c.begin + (j + 1) * B, c.end) - 1;
            used = t0 + last * (double)(j + 1) - begin;
            printf("rendering: %ux4 sampled (last %.3f sec). total: %.3f sec (%.2f %%).\n", sampled, last, used, used / time_limit * 100.0);
        }
        in_flight -= n;
        last_progress = now;
        used = now - begin;
        return 0;
    };
    // renderer.rs:222-241: the final image takes the current counter
    auto finish = [&](const char *why) -> int {
        for (uint32_t r = 0; r < ndev; r++)
            if (hr_synchronize(ctxs[r]) != 0) { fprintf(stderr, "hr_synchronize: %s\n", hr_last_error()); return 1; }
        printf("%s\n", why);
        printf("output final image: %03u.png\n", counter);
        printf("remain: %.3f sec.\n", time_limit - used);
        final_image = true;
        return save(sampled);
    };
    // how many reports may be enqueued now?  (samplings left, room in the pipeline, and the time-limit rule asked for the moment they would finish)
    const size_t depth = interval <= 0.0 ? 1 : (size_t)inflight;
    // --noise-target: nothing is issued beyond the sampling at which the next question is due (whole launches: the launch that
    // reaches it is not cut), so that a render that has reached its target stops there and not a pipeline's depth later
    // --adaptive asks at the same points: the tiles are chosen again, and the render ends when none is left.  Resumed with per-pixel counts it
    // asks before it renders anything: a tile that was done when the checkpoint was written is still done (its moments have not moved).
    const bool checks = have_target || have_adaptive;
    uint64_t check_at = (uint64_t)first - 1 + (resumed_counts && have_adaptive ? 0u : (uint64_t)noise_check);
    const uint32_t all_tiles = ((out_w + 3) / 4) * ((out_h + 3) / 4);
    auto may_issue = [&]() -> uint32_t {
        if (next_s > sampling || q.size() >= depth) return 0;
        if (checks && (uint64_t)next_s > check_at) return 0;
        uint32_t n = std::min<uint32_t>(lrep, reports_of(next_s, sampling + 1));
        // --adaptive: a launch ends where the tiles are chosen again (the uniform first phase is --noise-check samplings long, not a launch)
        if (have_adaptive) n = std::min<uint32_t>(n, std::max<uint32_t>(1, reports_of(next_s, (uint32_t)std::min<uint64_t>(check_at, sampling) + 1)));
        if (!measured) return n;   // nothing measured yet: fill the pipeline
        const double room = time_limit - (now_sec() - begin);
        const double fit = last > 0.0 ? room / (1.1 * last) - (double)in_flight : (room >= 0.0 ? (double)n : 0.0);
        if (fit < 1.0) return 0;
        return fit < (double)n ? (uint32_t)fit : n;
    };
    if (first > sampling && !debug && sampled > 0) {   // resumed from a checkpoint that already holds every requested sampling: just resolve it
        printf("reached max sampling\n");
        final_image = true;
        if (save(sampled)) return 1;
    }
    bool running = first <= sampling;
    while (running) {
        for (uint32_t n; (n = may_issue()) != 0;) if (issue(n)) return 1;
        if (q.empty() && have_adaptive && next_s <= sampling && (uint64_t)next_s > check_at) {   // the tiles are chosen again, and nothing is in flight
            uint32_t active = all_tiles;
            const int rc = hr_select_tiles(ctx, noise_floor, adaptive_e, &active);   // (HR_ERR_INVALID: a pixel with fewer than 2 samplings — no estimate yet, go on as before)
            if (rc != 0 && rc != HR_ERR_INVALID) { fprintf(stderr, "hr_select_tiles: %s\n", hr_last_error()); return 1; }
            if (rc == 0) {
                printf("adaptive: samplings=%u active=%u tiles=%u\n", next_s - 1, active, all_tiles);
                if (!active) { if (finish("no tile is active")) return 1; break; }
            }
            check_at = (uint64_t)next_s - 1 + (uint64_t)noise_check;
            continue;
        }
        if (q.empty() && have_target && next_s <= sampling && (uint64_t)next_s > check_at) {   // the question is due, and nothing is in flight
            if (noise_check_now()) return 1;
            if (noise_known && noise_last.mean_error <= noise_target) { if (finish("reached noise target")) return 1; break; }
            check_at = (uint64_t)next_s - 1 + (uint64_t)noise_check;
            continue;
        }
        if (q.empty()) {   // nothing in flight and nothing may follow: the render ends here (renderer.rs:222-241, the time limit asked first)
            // (samplings left over: only the time-limit rule can have refused them)
            if (finish(next_s <= sampling || used + 1.1 * last > time_limit ? "reached time limit" : "reached max sampling")) return 1;
            break;
        }
        if (report()) return 1;
        if (last_progress - last_image >= interval) {   // renderer.rs:243-251, with the `now` of the report
            while (!q.empty()) if (report()) return 1;   // the launches in flight: the image then holds exactly the samplings reported
            // nothing is in flight now: the reference's own rules apply as they stand, in their order (renderer.rs:222-241)
            if (used + 1.1 * last > time_limit) { if (finish("reached time limit")) return 1; break; }
            if (sampled >= sampling) { if (finish("reached max sampling")) return 1; break; }
            for (uint32_t r = 0; r < ndev; r++) CHECK_HR(hr_synchronize(ctxs[r]));
            printf("output progress image: %03u.png\n", counter);
            if (save(sampled)) return 1;
            counter++;
            last_image = last_progress;             // `now` of the report that triggered it (renderer.rs:250)
        }
    }
    for (uint32_t r = 0; r < ndev; r++) CHECK_HR(hr_synchronize(ctxs[r]));
    if (!ckpt_out.empty()) {
        std::vector<float> acc((size_t)out_w * out_h * 3);
        if (combine()) { fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
        if (host_sum) acc = sum_acc;
        else CHECK_HR(hr_read_accumulator(ctx, acc.data()));
        uint32_t hdr[9] = {has_region ? CKPT_REGION_MAGIC : CKPT_MAGIC, width, height, sampled, scene_hash, region[0], region[1], out_w, out_h};
        const size_t nhdr = has_region ? 9 : 5;
        FILE *f = fopen(ckpt_out.c_str(), "wb");
        bool ok = f && fwrite(hdr, 4, nhdr, f) == nhdr && fwrite(acc.data(), sizeof(float), acc.size(), f) == acc.size();
        if (ok && moments) {   // the trailer; a file written without moments keeps the bytes it always had
            hr_noise est;
            std::vector<double> mom;
            uint64_t mom_n = 0;
            if (noise_query(&est, nullptr, &mom, &mom_n) == 1) { fclose(f); fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
            ok = fwrite(&CKPT_MOMENTS_MAGIC, 4, 1, f) == 1 && fwrite(&mom_n, 8, 1, f) == 1 && fwrite(mom.data(), sizeof(double), mom.size(), f) == mom.size();
        }
        if (ok && counts) {   // behind the moments trailer (a render without moments: behind the accumulator)
            std::vector<uint32_t> cnt((size_t)out_w * out_h);
            if (hr_read_sample_counts(ctx, cnt.data()) != 0) { fclose(f); fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
            ok = fwrite(&CKPT_COUNTS_MAGIC, 4, 1, f) == 1 && fwrite(cnt.data(), sizeof(uint32_t), cnt.size(), f) == cnt.size();
        }
        if (ok && robust_k) {   // behind every other trailer; a file written without --robust keeps the bytes it always had
            std::vector<double> bkt((size_t)out_w * out_h * 3 * (size_t)robust_k);
            uint64_t bkt_n = 0;
            const uint32_t k32 = (uint32_t)robust_k;
            if (hr_read_buckets(ctx, bkt.data(), &bkt_n) != 0) { fclose(f); fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
            ok = fwrite(&CKPT_BUCKETS_MAGIC, 4, 1, f) == 1 && fwrite(&k32, 4, 1, f) == 1 && fwrite(&bkt_n, 8, 1, f) == 1 && fwrite(bkt.data(), sizeof(double), bkt.size(), f) == bkt.size();
        }
        if (f) fclose(f);
        if (!ok) { fprintf(stderr, "cannot write checkpoint %s\n", ckpt_out.c_str()); return 1; }
    }
    {   // main.rs:1217: result.png = the final image — the bytes finish() has just written as NNN.png
        bool copied = false;
        if (!last_png.empty()) {
            FILE *in = fopen(last_png.c_str(), "rb"), *out = in ? fopen("result.png", "wb") : nullptr;
            if (in && out) {
                std::vector<char> buf(1 << 20);
                size_t n;
                copied = true;
                while ((n = fread(buf.data(), 1, buf.size(), in)) > 0) copied = copied && fwrite(buf.data(), 1, n, out) == n;
                copied = copied && !ferror(in);
            }
            if (in) fclose(in);
            if (out) copied = (fclose(out) == 0) && copied;
        }
        if (!copied && hh_write_png_rgb8("result.png", rgb.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
    }
    if (moments) {   // the estimate of the final image, to result.txt as well; and its map
        std::vector<double> e_img(noise_png.empty() ? 0 : (size_t)out_w * out_h);
        int rc = noise_query(&noise_last, e_img.empty() ? nullptr : e_img.data(), nullptr, nullptr);
        if (rc == 1) { fprintf(stderr, "hr_noise_estimate: %s\n", hr_last_error()); return 1; }
        if (rc == 2) tee("noise: fewer than 2 samplings, no estimate.");
        else tee("noise: samplings=%llu mean=%.9g max=%.9g above=%llu", (unsigned long long)noise_last.samplings, noise_last.mean_error, noise_last.max_error,
                 (unsigned long long)noise_last.pixels_above);
        if (!noise_png.empty() && rc == 0) {   // grey map of min(1, e / E)
            const double E = noise_e > 0.0 ? noise_e : 0.05;
            std::vector<uint8_t> grey((size_t)out_w * out_h * 3);
            for (size_t i = 0; i < e_img.size(); i++) {
                const double t = e_img[i] / E;
                const uint8_t v = (uint8_t)((t >= 1.0 ? 1.0 : (t > 0.0 ? t : 0.0)) * 255.0 + 0.5);
                grey[i * 3] = grey[i * 3 + 1] = grey[i * 3 + 2] = v;
            }
            if (hh_write_png_rgb8(noise_png.c_str(), grey.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
        }
    }
    if (!guide_prefix.empty()) {   // the guide planes as images of their own (the planes of --denoise's filter, or a pass of their own)
        std::vector<float> g((size_t)out_w * out_h * 8);
        if (!have_guides) CHECK_HR(hr_render_guides(ctx));
        CHECK_HR(hr_read_guides(ctx, g.data()));
        const size_t pixels = (size_t)out_w * out_h;
        float zmax = 0.0f;
        for (size_t i = 0; i < pixels; i++) zmax = std::max(zmax, g[i * 8 + 6]);
        auto byte = [](float v) { return (uint8_t)(std::min(1.0f, std::max(0.0f, v)) * 255.0f + 0.5f); };
        std::vector<uint8_t> img(pixels * 3);
        for (size_t i = 0; i < pixels; i++) for (int k = 0; k < 3; k++) img[i * 3 + k] = byte(powf(std::max(0.0f, g[i * 8 + k]), 1.0f / 2.2f));
        if (hh_write_png_rgb8((guide_prefix + "_albedo.png").c_str(), img.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
        for (size_t i = 0; i < pixels; i++) for (int k = 0; k < 3; k++) img[i * 3 + k] = byte(0.5f * g[i * 8 + 3 + k] + 0.5f * g[i * 8 + 7]);
        if (hh_write_png_rgb8((guide_prefix + "_normal.png").c_str(), img.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
        for (size_t i = 0; i < pixels; i++) img[i * 3] = img[i * 3 + 1] = img[i * 3 + 2] = byte(zmax > 0.0f ? g[i * 8 + 6] / zmax : 0.0f);
        if (hh_write_png_rgb8((guide_prefix + "_depth.png").c_str(), img.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
    }
    if (robust_k) {   // how much the robust resolve dropped; and its map
        std::vector<uint8_t> trim((size_t)out_w * out_h);
        CHECK_HR(hr_robust(ctx));
        CHECK_HR(hr_read_robust_trim(ctx, trim.data()));
        const uint32_t most = (uint32_t)(robust_k - 1) / 2;
        size_t trimmed = 0;
        for (uint8_t v : trim) trimmed += v != 0;
        tee("robust: buckets=%lld trimmed pixels=%.4f", robust_k, (double)trimmed / (double)trim.size());
        if (!robust_png.empty()) {   // grey map of trim / ((K - 1) / 2)
            std::vector<uint8_t> grey(trim.size() * 3);
            for (size_t i = 0; i < trim.size(); i++) grey[i * 3] = grey[i * 3 + 1] = grey[i * 3 + 2] = (uint8_t)((double)trim[i] / (double)most * 255.0 + 0.5);
            if (hh_write_png_rgb8(robust_png.c_str(), grey.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
        }
    }
    if (counts) {   // how the samplings were spent
        std::vector<uint32_t> cnt((size_t)out_w * out_h);
        CHECK_HR(hr_read_sample_counts(ctx, cnt.data()));
        uint32_t lo = ~0u, hi = 0;
        uint64_t sum = 0;
        for (uint32_t v : cnt) { lo = std::min(lo, v); hi = std::max(hi, v); sum += v; }
        tee("samplings per pixel: min=%u max=%u mean=%.3f", lo, hi, (double)sum / (double)cnt.size());
        if (!sample_png.empty()) {   // grey map of count / largest count
            std::vector<uint8_t> grey(cnt.size() * 3);
            for (size_t i = 0; i < cnt.size(); i++) grey[i * 3] = grey[i * 3 + 1] = grey[i * 3 + 2] = hi ? (uint8_t)((double)cnt[i] / (double)hi * 255.0 + 0.5) : 0;
            if (hh_write_png_rgb8(sample_png.c_str(), grey.data(), out_w, out_h) != 0) { fprintf(stderr, "png: %s\n", hh_last_error()); return 1; }
        }
    }
    tee("sampled: %ux%u spp.", sampled, 4u);
    hr_stats st;
    if (hr_get_stats(ctx, &st) == 0) {
        double sec = st.trace_kernel_ms * 1e-3;
        uint64_t paths = st.paths;
        for (uint32_t r = 1; r < ndev; r++) { hr_stats o; if (hr_get_stats(ctxs[r], &o) == 0) paths += o.paths; }
        // two clocks: until the last sampling was reported (the render itself), and until here (+ the final hr_resolve and the PNG encoder)
        tee("gpu: %.3f Mpaths/s wall (%.3f incl. the final image), trace kernel %.3f s, seed kernel %.3f s.", (double)paths / std::max(1e-9, last_progress - begin) * 1e-6,
            (double)paths / (now_sec() - begin) * 1e-6, sec, st.seed_kernel_ms * 1e-3);
    }
    double total = now_sec() - total_begin;
    double used_percent = total / time_limit * 100.0;
    tee("total %g sec. used %.2f %% (x %.2f)", total, used_percent, 100.0 / used_percent);
    for (hr_ctx *c : ctxs) hr_destroy(c);
    hh_scene_destroy(scene);
    if (g_log) fclose(g_log);
    return 0;
}
