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
// the guide rays follow mirrors and glass for up to K bounces to the first rough hit; 0, the default, is the first hit), --guide-lens L
// (hr_render_guides_lens: the guide planes averaged over 4 or 16 fixed points of the thin lens, rendered once when the devices are opened),
// --robust K / --robust-image FILE (option "robust_buckets": every image is the firefly-robust resolve of K sample buckets per pixel, hr_robust +
// hr_resolve_robust; the buckets ride in the checkpoint behind the other trailers),
// --robust-noise (with --robust: --noise-target, --adaptive and --noise-image judge the robust image by the spread of its bucket means,
// hr_robust_noise_estimate / hr_select_tiles_robust / hr_read_robust_noise_image), --robust-denoise (with --robust: the FINAL
// image is the a-trous filter's over the robust radiance and its bucket-spread variance, hr_denoise_robust + hr_resolve_denoised),
// --robust-restore / --restore-levels N (with --robust: the FINAL image is the robust radiance — with --robust-denoise the denoised one — plus the
// trimmed buckets' excess spread along the guide planes, hr_robust_restore + hr_resolve_restored),
// --denoise-auto K / --select-smooth N / --level-image FILE (options "moments" and "robust_buckets": the FINAL image is --denoise's filter with the
// level picked per pixel from the held-out halves of the K sample buckets, hr_denoise_select + hr_resolve_selected),
// --auto-noise (with --denoise-auto: --noise-target, --adaptive and --noise-image judge the image --denoise-auto shows by its estimated error,
// hr_selected_noise_estimate / hr_select_tiles_selected / hr_read_selected_noise_image).
// The file is in main's order: Options and parse_options (everything that can be refused before a device is opened), then Run, whose members
// are main's steps.  The checkpoint's format is host/checkpoint.h's; what a render demands of a file is said in Run::resume.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "checkpoint.h"
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
           "        --guide-lens L  average the guide planes over L = 4 or 16 fixed points of the camera's thin lens (hr_render_guides_lens), so that\n"
           "                        they are as soft as the image where it is out of focus; about L times the pinhole pass.  A scene without an\n"
           "                        aperture gets the pinhole planes.  Works with --guide-bounces.  Needs --denoise, --robust-denoise,\n"
           "                        --robust-restore, --denoise-auto or --guide-image.\n"
           "        --robust K      keep K sample buckets per pixel (K odd, 3 .. 15; 3 K doubles per pixel) and write every image, progress and final,\n"
           "                        through the firefly-robust resolve (hr_robust + hr_resolve_robust: an adaptive median of the K bucket means, which\n"
           "                        drops the buckets a few very bright paths landed in; biased dark where it trims).  Works with --region,\n"
           "                        --noise-target and --adaptive (every pixel's own sampling count).  --checkpoint appends the buckets, --resume\n"
           "                        restores them and refuses a file without them or with another K.  One device only; not with --denoise or --debug.\n"
           "        --robust-image FILE.png\n"
           "                        write an 8-bit grey map of trim / ((K - 1) / 2), the buckets dropped at either end (needs --robust)\n"
           "        --robust-noise  judge the noise of the image --robust shows, not of the plain mean: --noise-target asks hr_robust_noise_estimate,\n"
           "                        --adaptive asks hr_select_tiles_robust (after --resume too) and --noise-image maps min(1, e_R / E), e_R the\n"
           "                        winsorized standard error of the trimmed mean of the K bucket means over the channel sum + 3 F.  No estimate\n"
           "                        before every pixel has K samplings.  Needs --robust; without this flag everything is judged as before.\n"
           "        --robust-denoise\n"
           "                        write the FINAL image through the a-trous filter on the robust radiance (hr_denoise_robust: --denoise's filter, fed\n"
           "                        with the trimmed mean of the K bucket means and the winsorized variance of their spread instead of the raw moments;\n"
           "                        progress images stay --robust's).  --denoise-levels, --guide-bounces and --guide-image work as with --denoise.  A\n"
           "                        pixel with fewer than K samplings: the robust image is written unfiltered.  Needs --robust.\n"
           "        --robust-restore\n"
           "                        write the FINAL image with the energy the robust resolve drops given back (hr_robust_restore: what the trimmed hot\n"
           "                        buckets hold above the highest kept one is spread over the neighbourhood along the guide planes and added; the image\n"
           "                        keeps the brightness of the plain mean at a larger error than --robust alone; progress images stay --robust's).\n"
           "                        With --robust-denoise the excess goes on top of the denoised image.  --guide-bounces works as with --denoise.  A\n"
           "                        pixel with fewer than K samplings: the image is written unrestored.  Needs --robust.\n"
           "        --restore-levels N\n"
           "                        spread levels, 0 .. 5 (default 4; the taps of level l are 2^l pixels apart).  Needs --robust-restore.\n"
           "        --denoise-auto K\n"
           "                        keep per-pixel sample moments and K sample buckets (K odd, 3 .. 15) and write the FINAL image through --denoise's\n"
           "                        filter with the level picked PER PIXEL, 0 .. --denoise-levels (hr_denoise_select: the two halves of the buckets are\n"
           "                        filtered apart and each is judged against the raw pixel of the other; progress images stay as they are).\n"
           "                        --denoise-levels, --guide-bounces and --guide-image work as with --denoise.  A pixel with fewer than 2 samplings,\n"
           "                        or a --resume whose checkpoint has no buckets: the image is written unfiltered.  One device only; not with\n"
           "                        --robust, --denoise or --debug.\n"
           "        --select-smooth N\n"
           "                        smoothing passes over the per-level error planes before the pick, 0 .. 3 (default 2).  Needs --denoise-auto.\n"
           "        --auto-noise    judge the noise of the image --denoise-auto shows, not of the plain mean: --noise-target asks\n"
           "                        hr_selected_noise_estimate, --adaptive asks hr_select_tiles_selected and --noise-image maps min(1, e_S / E), e_S the\n"
           "                        estimated relative error of the selected radiance (a propagated variance plus a held-out bias), with this run's\n"
           "                        --denoise-levels and --select-smooth.  Needs --denoise-auto; one device; not with --robust-noise or --resume.\n"
           "        --level-image FILE.png\n"
           "                        write an 8-bit grey map of level / --denoise-levels, the level each pixel took (needs --denoise-auto)\n"
           "        --frames N      render N frames of -s samplings each and write them as frame_000.png .. (hr_set_camera between them: the scene is\n"
           "                        uploaded and its tree built once).  Frame f renders samplings f S + 1 .. (f + 1) S and prints one \"frame f:\" line.\n"
           "                        One device; only with -w -h -s --scene --assets --precise / --no-precise --denoise --denoise-levels --guide-bounces.\n"
           "        --orbit DEG     degrees per frame: the camera turns about the vertical axis through its focus point (default 0).  Needs --frames.\n"
           "        --temporal M    every frame after the first starts from the frame before it, reprojected along a motion plane (hr_render_motion of\n"
           "                        the previous camera, hr_reproject), with at most M samplings of history per pixel.  Needs --frames.\n",
           prog);
}

struct Options {
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
    long long guide_lens = 0;        // --guide-lens L: 4 or 16 lens points behind every guide value (0: not given, pinhole planes)
    long long robust_k = 0;          // --robust K: option "robust_buckets" (0: off)
    std::string robust_png;
    bool robust_noise = false;       // --robust-noise: the noise questions are asked of the buckets (e_R), not of the moments
    bool robust_denoise = false;     // --robust-denoise: the final image is hr_denoise_robust's
    bool robust_restore = false;     // --robust-restore: the final image is hr_robust_restore's
    long long restore_levels = -1;   // -1: the library's default
    long long auto_k = 0;            // --denoise-auto K: options "moments" and "robust_buckets", the final image is hr_denoise_select's (0: off)
    long long select_smooth = -1;    // -1: the library's default
    bool auto_noise = false;         // --auto-noise: the noise questions are asked of the image --denoise-auto shows (e_S), not of the moments
    std::string level_png;
    long long frames = 0;            // --frames N: a sequence of N frames (0: one image, as always)
    double orbit_deg = 0.0;          // --orbit DEG: degrees per frame about the vertical axis through the focus point
    long long temporal = 0;          // --temporal M: hr_reproject's max_history (0: every frame starts from nothing)
    bool have_orbit = false;
    std::string beyond_frames;       // the first flag given that --frames does not go with
    // what the flags add up to:
    bool counts = false, moments = false;   // hr_set_option "sample_counts", "moments"
    double noise_e = 0.05;                  // the threshold of "above" and of the grey map
    uint32_t region[4] = {0, 0, 0, 0};      // --region, or the whole frame
    bool has_region = false;
    uint32_t out_w = 0, out_h = 0;          // the accumulator and the images: the region's
};

// a number, the whole argument, not NaN; what is wrong with it is said with the flag's name, before any device is opened
static bool number(const char *flag, const char *text, double *out) {
    char *e = nullptr;
    *out = strtod(text, &e);
    if (e == text || *e || std::isnan(*out) || std::isinf(*out)) { fprintf(stderr, "%s: '%s' is not a number.\n", flag, text); return false; }
    return true;
}
// a whole number, the whole argument, one of lo, lo + step, .. up to hi; `what` is the flag's own word for that
static bool whole(const char *flag, const char *text, long long lo, long long hi, long long step, const char *what, long long *out) {
    char *e = nullptr;
    *out = strtoll(text, &e, 10);
    if (e == text || *e || *out < lo || *out > hi || (*out - lo) % step) { fprintf(stderr, "%s must be %s, not '%s'.\n", flag, what, text); return false; }
    return true;
}
// a feature that this program renders on one device only: its sentence, when --gpus / --gpu-ids name more
static bool one_device(const Options &o, const char *sentence) {
    size_t ids = o.gpu_ids.empty() ? 0 : 1;
    for (char ch : o.gpu_ids) ids += ch == ',';
    if (o.gpus > 1 || ids > 1) fprintf(stderr, "%s\n", sentence);
    return !(o.gpus > 1 || ids > 1);
}
// --region X,Y,W,H: four unsigned integers, a non-empty window inside the frame (hr_set_region's rule, checked before any device is opened)
static bool parse_region(const char *text, uint32_t width, uint32_t height, uint32_t region[4]) {
    uint64_t v[4];
    int n = 0;
    for (const char *p = text; n < 4; n++) {
        if (*p < '0' || *p > '9') break;
        char *e = nullptr;
        v[n] = strtoull(p, &e, 10);
        if (v[n] > 0xffffffffull) break;
        p = e;
        if (n < 3 && *p++ != ',') break;
        if (n == 3 && *p) break;
    }
    if (n != 4) { fprintf(stderr, "--region must be X,Y,W,H (four unsigned integers), not '%s'.\n", text); return false; }
    if (!v[2] || !v[3] || v[0] > width || v[2] > width - v[0] || v[1] > height || v[3] > height - v[1]) {
        fprintf(stderr, "--region %s: the window must be non-empty and lie inside the %ux%u frame.\n", text, width, height);
        return false;
    }
    for (int k = 0; k < 4; k++) region[k] = (uint32_t)v[k];
    return true;
}

// argv into Options, with every refusal that needs no device.  Returns the exit status, or -1: go on and render.
static int parse_options(int argc, char **argv, Options &o) {
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "Argument to option '%s' missing.\n", name); exit(1); }
            return argv[++i];
        };
        if (a == "--help") { usage(argv[0]); return 0; }
        {
            static const char *const with_frames[] = {"-w", "--width", "-h", "--height", "-s", "--sampling", "--scene", "--assets", "--precise", "--no-precise", "--denoise",
                                                      "--denoise-levels", "--guide-bounces", "--frames", "--orbit", "--temporal"};
            bool known = false;
            for (const char *f : with_frames) known = known || a == f;
            if (!known && o.beyond_frames.empty()) o.beyond_frames = a;
        }
        if (a == "--frames") {
            if (!whole("--frames", val("frames"), 1, 999, 1, "a whole number of frames in 1 .. 999", &o.frames)) return 1;
        } else if (a == "--orbit") {
            if (!number("--orbit", val("orbit"), &o.orbit_deg)) return 1;
            o.have_orbit = true;
        } else if (a == "--temporal") {
            if (!whole("--temporal", val("temporal"), 1, 0x7fffffffll, 1, "a whole number of samplings, at least 1", &o.temporal)) return 1;
        }
        else if (a == "-d" || a == "--debug") o.debug = true;
        else if (a == "-w" || a == "--width") o.width = (uint32_t)strtoul(val("w"), nullptr, 10);
        else if (a == "-h" || a == "--height") o.height = (uint32_t)strtoul(val("h"), nullptr, 10);
        else if (a == "-s" || a == "--sampling") o.sampling = (uint32_t)strtoul(val("s"), nullptr, 10);
        else if (a == "-t" || a == "--time") o.time_limit = strtod(val("t"), nullptr);
        else if (a == "-i" || a == "--interval") o.interval = strtod(val("i"), nullptr);
        else if (a == "--scene") o.scene_name = val("scene");
        else if (a == "--assets") o.assets = val("assets");
        else if (a == "--batch") o.batch = atoi(val("batch"));
        else if (a == "--launch") o.launch = atoi(val("launch"));
        else if (a == "--inflight") o.inflight = atoi(val("inflight"));
        else if (a == "--precise") o.precise = 1;
        else if (a == "--no-precise") o.precise = 0;
        else if (a == "--gpus") o.gpus = atoi(val("gpus"));
        else if (a == "--gpu-ids") o.gpu_ids = val("gpu-ids");
        else if (a == "--checkpoint") o.ckpt_out = val("checkpoint");
        else if (a == "--resume") o.ckpt_in = val("resume");
        else if (a == "--region") o.region_arg = val("region");
        else if (a == "--noise-target") {
            if (!number("--noise-target", val("noise-target"), &o.noise_target)) return 1;
            if (o.noise_target < 0.0) { fprintf(stderr, "--noise-target must not be negative.\n"); return 1; }
            o.have_target = true;
        } else if (a == "--noise-floor") {
            if (!number("--noise-floor", val("noise-floor"), &o.noise_floor)) return 1;
            if (!(o.noise_floor > 0.0)) { fprintf(stderr, "--noise-floor must be positive.\n"); return 1; }
        } else if (a == "--noise-check") {
            if (!whole("--noise-check", val("noise-check"), 1, 0x7fffffffll, 1, "a whole number of samplings, at least 1", &o.noise_check)) return 1;
        } else if (a == "--noise-image") o.noise_png = val("noise-image");
        else if (a == "--adaptive") {
            if (!number("--adaptive", val("adaptive"), &o.adaptive_e)) return 1;
            if (!(o.adaptive_e > 0.0)) { fprintf(stderr, "--adaptive must be positive.\n"); return 1; }
            o.have_adaptive = true;
        } else if (a == "--sample-image") o.sample_png = val("sample-image");
        else if (a == "--denoise") o.denoise = true;
        else if (a == "--denoise-levels") {
            if (!whole("--denoise-levels", val("denoise-levels"), 0, 5, 1, "a whole number in 0 .. 5", &o.denoise_levels)) return 1;
        } else if (a == "--guide-image") o.guide_prefix = val("guide-image");
        else if (a == "--guide-bounces") {
            if (!whole("--guide-bounces", val("guide-bounces"), 0, 8, 1, "a whole number in 0 .. 8", &o.guide_bounces)) return 1;
        } else if (a == "--guide-lens") {
            if (!whole("--guide-lens", val("guide-lens"), 4, 16, 12, "4 or 16", &o.guide_lens)) return 1;
        } else if (a == "--robust") {
            if (!whole("--robust", val("robust"), 3, 15, 2, "an odd number of buckets in 3 .. 15", &o.robust_k)) return 1;
        } else if (a == "--robust-image") o.robust_png = val("robust-image");
        else if (a == "--robust-noise") o.robust_noise = true;
        else if (a == "--robust-denoise") o.robust_denoise = true;
        else if (a == "--robust-restore") o.robust_restore = true;
        else if (a == "--denoise-auto") {
            if (!whole("--denoise-auto", val("denoise-auto"), 3, 15, 2, "an odd number of buckets in 3 .. 15", &o.auto_k)) return 1;
        } else if (a == "--select-smooth") {
            if (!whole("--select-smooth", val("select-smooth"), 0, 3, 1, "a whole number in 0 .. 3", &o.select_smooth)) return 1;
        } else if (a == "--level-image") o.level_png = val("level-image");
        else if (a == "--auto-noise") o.auto_noise = true;
        else if (a == "--restore-levels") {
            if (!whole("--restore-levels", val("restore-levels"), 0, 5, 1, "a whole number in 0 .. 5", &o.restore_levels)) return 1;
        }
        else { fprintf(stderr, "Unrecognized option: '%s'.\n", a.c_str()); return 1; }
    }
    if (!o.frames && (o.have_orbit || o.temporal)) { fprintf(stderr, "--orbit / --temporal need --frames.\n"); return 1; }
    if (o.frames && !o.beyond_frames.empty()) {
        fprintf(stderr, "--frames cannot be combined with %s: a sequence renders on one device, from nothing, with -w -h -s --scene --assets --precise / --no-precise --denoise --denoise-levels --guide-bounces only.\n",
                o.beyond_frames.c_str());
        return 1;
    }
    if (o.frames && (!o.sampling || o.sampling > 0xffffffffu / (uint32_t)o.frames)) { fprintf(stderr, "--frames: -s samplings per frame must be positive and N x S must fit 32 bits.\n"); return 1; }
    if (o.batch < 1) { fprintf(stderr, "--batch must be at least 1.\n"); return 1; }
    if (o.launch < 0) { fprintf(stderr, "--launch must be at least 1 (or 0: automatic).\n"); return 1; }
    if (o.inflight < 1) { fprintf(stderr, "--inflight must be at least 1.\n"); return 1; }
    if (o.width == 0 || o.height == 0) { fprintf(stderr, "width and height must be positive.\n"); return 1; }
    if (o.gpus < 1) { fprintf(stderr, "--gpus must be at least 1.\n"); return 1; }
    o.counts = o.have_adaptive || !o.sample_png.empty() || o.frames != 0;   // (a sequence resolves every frame with the pixels' own counts)
    if (o.counts) {
        if (!one_device(o, "--adaptive / --sample-image render on one device: the library can shard an adaptive render (masks and additive counts), this program's device loop does not.")) return 1;
        if (o.have_adaptive && o.have_target) { fprintf(stderr, "--adaptive and --noise-target are two stop rules: give one of them.\n"); return 1; }
        if (o.debug) { fprintf(stderr, "--adaptive / --sample-image cannot be combined with --debug (the debug renderer has no samplings to count).\n"); return 1; }
    }
    if (o.auto_noise) {   // (before --denoise-auto's own: every refusal of this flag names it)
        if (!o.auto_k) { fprintf(stderr, "--auto-noise needs --denoise-auto (it judges the noise of the image --denoise-auto shows).\n"); return 1; }
        if (o.robust_noise) { fprintf(stderr, "--auto-noise cannot be combined with --robust-noise (two images to judge the noise of).\n"); return 1; }
        if (!o.ckpt_in.empty()) { fprintf(stderr, "--auto-noise cannot be combined with --resume (the checkpoint does not carry the sample buckets --denoise-auto keeps).\n"); return 1; }
        if (!one_device(o, "--auto-noise renders on one device, as --denoise-auto does: the library estimates from one context's moments and sample buckets.")) return 1;
    }
    if (o.auto_k) {   // before everything else about these flags: nothing of --denoise-auto is half accepted
        if (o.robust_k) { fprintf(stderr, "--denoise-auto cannot be combined with --robust (it filters the plain mean, and keeps sample buckets of its own: two final images).\n"); return 1; }
        if (o.denoise) { fprintf(stderr, "--denoise-auto cannot be combined with --denoise (one filter with one level for the frame, one with a level per pixel: two final images).\n"); return 1; }
        if (o.debug) { fprintf(stderr, "--denoise-auto cannot be combined with --debug (the debug renderer has no samplings to split into halves).\n"); return 1; }
        if (!one_device(o, "--denoise-auto renders on one device: the library picks the levels from one context's moments and sample buckets, this program's device loop does not fold them.")) return 1;
    }
    if (o.select_smooth >= 0 && !o.auto_k) { fprintf(stderr, "--select-smooth needs --denoise-auto.\n"); return 1; }
    if (!o.level_png.empty() && !o.auto_k) { fprintf(stderr, "--level-image needs --denoise-auto.\n"); return 1; }
    if (o.robust_denoise && !o.robust_k) { fprintf(stderr, "--robust-denoise needs --robust (it filters the robust radiance by the spread of the sample buckets).\n"); return 1; }
    if (o.robust_restore && !o.robust_k) { fprintf(stderr, "--robust-restore needs --robust (it gives back the energy the robust resolve drops).\n"); return 1; }
    if (o.restore_levels >= 0 && !o.robust_restore) { fprintf(stderr, "--restore-levels needs --robust-restore.\n"); return 1; }
    if (o.denoise_levels >= 0 && !o.denoise && !o.robust_denoise && !o.auto_k) { fprintf(stderr, "--denoise-levels needs --denoise.\n"); return 1; }
    if (o.guide_lens && !o.denoise && !o.robust_denoise && !o.robust_restore && !o.auto_k && o.guide_prefix.empty()) { fprintf(stderr, "--guide-lens needs --denoise, --robust-denoise, --robust-restore, --denoise-auto or --guide-image.\n"); return 1; }
    if (o.guide_bounces >= 0 && !o.denoise && !o.robust_denoise && !o.robust_restore && !o.auto_k && o.guide_prefix.empty()) { fprintf(stderr, "--guide-bounces needs --denoise or --guide-image.\n"); return 1; }
    if (o.denoise || !o.guide_prefix.empty()) {
        if (!one_device(o, "--denoise / --guide-image render on one device: the library denoises one context's accumulator, moments and counts (a sharded host sums them into one), this program's device loop does not.")) return 1;
        if (o.debug) { fprintf(stderr, "--denoise / --guide-image cannot be combined with --debug (the debug renderer has no samplings whose variance could guide a filter).\n"); return 1; }
    }
    if (!o.robust_png.empty() && !o.robust_k) { fprintf(stderr, "--robust-image needs --robust.\n"); return 1; }
    if (o.robust_noise && !o.robust_k) { fprintf(stderr, "--robust-noise needs --robust (it judges the noise by the sample buckets).\n"); return 1; }
    if (o.robust_k) {
        if (!one_device(o, "--robust renders on one device: buckets of several devices add up only when each rendered a multiple of K samplings, and this program's device loop does not see to that.")) return 1;
        if (o.denoise) { fprintf(stderr, "--robust cannot be combined with --denoise (the filter reads the raw moments, not the robust radiance: two final images).\n"); return 1; }
        if (o.debug) { fprintf(stderr, "--robust cannot be combined with --debug (the debug renderer has no samplings to put into buckets).\n"); return 1; }
    }
    o.moments = o.have_target || !o.noise_png.empty() || o.have_adaptive || o.denoise || o.auto_k != 0;
    if (o.moments && o.debug) { fprintf(stderr, "--noise-target / --noise-image cannot be combined with --debug (the debug renderer has no samplings to measure).\n"); return 1; }
    o.noise_e = o.have_adaptive ? o.adaptive_e : o.have_target && o.noise_target > 0.0 ? o.noise_target : (o.have_target ? 0.0 : 0.05);
    o.region[2] = o.width, o.region[3] = o.height;
    if (!o.region_arg.empty()) {
        if (!parse_region(o.region_arg.c_str(), o.width, o.height, o.region)) return 1;
        o.has_region = o.region[2] != o.width || o.region[3] != o.height;   // the whole frame as a region is no region
    }
    o.out_w = o.region[2], o.out_h = o.region[3];
    if (o.assets.empty()) {
        FILE *probe = fopen("assets/models/box.obj", "rb");
        if (probe) { fclose(probe); o.assets = "assets"; } else o.assets = ".";
    }
    return -1;
}

static int write_png(const std::string &path, const uint8_t *rgb, uint32_t w, uint32_t h) {
    if (hh_write_png_rgb8(path.c_str(), rgb, w, h) == 0) return 0;
    fprintf(stderr, "png: %s\n", hh_last_error());
    return 1;
}
// One value per pixel, in 0 .. 1 (the caller clamps where its values can leave that range), as an 8-bit grey PNG: v * 255 + 0.5, cut off, in
// the arithmetic of the values' own type (the depth plane's are floats, the others doubles).
template <class F> static int write_grey(const std::string &path, uint32_t w, uint32_t h, F value) {
    using T = decltype(value((size_t)0));
    std::vector<uint8_t> grey((size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; i++) grey[i * 3] = grey[i * 3 + 1] = grey[i * 3 + 2] = (uint8_t)(value(i) * (T)255.0 + (T)0.5);
    return write_png(path, grey.data(), w, h);
}

// One render: the devices, what has been rendered so far, and main's steps in their order.  Every step returns 0 or the exit status.
struct Run {
    const Options &o;
    uint32_t sampling;          // the render loop's limit: -s (0 once --debug has rendered its one image)
    uint32_t scene_hash = 2166136261u;   // FNV-1a of the scene name, for the checkpoint's header
    double total_begin = now_sec();
    hh_scene *scene = nullptr;
    std::vector<hr_ctx *> ctxs;
    hr_ctx *ctx = nullptr;      // device 0: it resolves the images
    uint32_t ndev = 0;
    bool host_sum = false;
    std::vector<float> sum_acc, part;
    bool have_guides = false;   // the context holds guide planes (for --guide-image)
    bool have_levels = false;   // the context holds a selected image and its level plane (for --level-image)
    uint32_t select_levels = 0; // the levels that selection could choose from
    bool final_image = false;   // set by whoever writes the render's last image: --denoise filters that one only
    std::vector<double> mom_tot, mom_part, mom_own;
    hr_noise noise_last;
    bool noise_known = false;
    std::vector<uint8_t> rgb;
    double begin = 0.0, last_progress = 0.0, last_image = 0.0;
    uint32_t counter = 0, sampled = 0;
    std::string last_png;       // the image file save() wrote last: result.png is a copy of the final one (one PNG encode, not two)
    uint32_t first = 1;
    bool resumed_counts = false;   // --resume restored per-pixel counts: the tiles are chosen again before anything is rendered

    explicit Run(const Options &opt) : o(opt), sampling(opt.sampling) {
        for (char ch : o.scene_name) scene_hash = (scene_hash ^ (uint8_t)ch) * 16777619u;
    }
    // main's steps, in its order
    void print_settings() const;
    int open_devices();
    int resume();
    int render();
    int render_frames();
    int write_checkpoint();
    int write_result_png();
    int write_reports();
    void close();
    // what the steps share
    int combine();
    int resolve(uint32_t s, uint8_t *out);
    int select_params(hr_denoise_params *dp, hr_select_params *sp);
    int noise_query(hr_noise *est, double *img, std::vector<double> *tot_out, uint64_t *n_out);
    int noise_check_now();
    int save(uint32_t s);
};

void Run::print_settings() const {
    tee("num threads: %d.", 1);  // main.rs:1261 prints rayon's pool size; here: one host thread drives one GPU
    tee("resolution: %ux%u.", o.width, o.height);
    if (o.has_region) tee("region: %u,%u %ux%u.", o.region[0], o.region[1], o.out_w, o.out_h);
    tee("max sampling: %ux%u spp.", o.sampling, 4u);
    tee("time limit: %.2f sec.", o.time_limit);
    tee("report interval: %.2f sec.", o.interval);
}

int Run::open_devices() {
    double init_begin = now_sec();
    if (hh_scene_create(o.scene_name.c_str(), o.assets.c_str(), &scene) != 0) { fprintf(stderr, "scene: %s\n", hh_last_error()); return 1; }
    // devices: samplings are independent and seeded by index, so device r of N renders samplings first + r, first + r + N, ...
    // (bench.py does the same with one process per GPU and an RCCL all-reduce)
    std::vector<int> devices;
    if (!o.gpu_ids.empty()) {
        for (size_t p = 0; p < o.gpu_ids.size();) {
            size_t q = o.gpu_ids.find(',', p);
            devices.push_back(atoi(o.gpu_ids.substr(p, q == std::string::npos ? std::string::npos : q - p).c_str()));
            if (q == std::string::npos) break;
            p = q + 1;
        }
    } else {
        for (int d = 0; d < (o.gpus > 0 ? o.gpus : 1); d++) devices.push_back(d);
    }
    ndev = (uint32_t)devices.size();
    ctxs.assign(ndev, nullptr);
    for (uint32_t r = 0; r < ndev; r++) {
        CHECK_HR(hr_create(devices[r], &ctxs[r]));
        CHECK_HR(hr_upload_scene(ctxs[r], hh_scene_desc(scene)));
        CHECK_HR(hr_set_resolution(ctxs[r], o.width, o.height));
        if (o.has_region) CHECK_HR(hr_set_region(ctxs[r], o.region[0], o.region[1], o.out_w, o.out_h));
        if (o.precise >= 0) CHECK_HR(hr_set_option(ctxs[r], "precise_shading", (double)o.precise));
        if (o.moments) CHECK_HR(hr_set_option(ctxs[r], "moments", 1.0));
        if (o.counts) CHECK_HR(hr_set_option(ctxs[r], "sample_counts", 1.0));
        if (o.guide_bounces >= 0) CHECK_HR(hr_set_option(ctxs[r], "guide_bounces", (double)o.guide_bounces));
        if (o.robust_k) CHECK_HR(hr_set_option(ctxs[r], "robust_buckets", (double)o.robust_k));
        if (o.auto_k) CHECK_HR(hr_set_option(ctxs[r], "robust_buckets", (double)o.auto_k));
    }
    ctx = ctxs[0];
    // --guide-lens: the planes are rendered here, once, where the library would otherwise render pinhole planes at the first call that needs them
    // (one device: checked with the flags; nothing this program does afterwards drops them)
    if (o.guide_lens) { CHECK_HR(hr_render_guides_lens(ctx, (uint32_t)o.guide_lens)); have_guides = true; }
    if (ndev > 1) tee("devices: %u.", ndev);
    tee("init scene: %.2f sec.", now_sec() - init_begin);
    // The image needs the sum of all devices' accumulators: ONE all-reduce over RCCL (hr_allreduce_accumulators — the sum lands
    // in a separate buffer per device, so every device keeps accumulating its own samplings afterwards); hr_resolve /
    // hr_read_accumulator on device 0 then see the total (renderer.rs:64-90 runs after the sum).
    // A multi-GPU box whose RCCL cannot be loaded (hr_comm_init_local: HR_ERR_UNSUPPORTED) still renders: the host then sums the
    // devices' accumulators itself when an image or a checkpoint is written (`sum_acc` below) — slower, same result.
    if (ndev > 1) {
        int rc = hr_comm_init_local(ctxs.data(), (int)ndev);
        if (rc == HR_ERR_UNSUPPORTED) { host_sum = true; tee("no RCCL (%s): accumulators are summed on the host.", hr_last_error()); }
        else if (rc != 0) { fprintf(stderr, "hr_comm_init_local: %s\n", hr_last_error()); return 1; }
    }
    rgb.resize((size_t)o.out_w * o.out_h * 3);
    begin = last_progress = last_image = now_sec();
    return 0;
}

int Run::combine() {
    if (ndev == 1) return 0;
    if (!host_sum) return hr_allreduce_accumulators(ctxs.data(), (int)ndev) != 0;
    sum_acc.resize((size_t)o.out_w * o.out_h * 3);
    part.resize(sum_acc.size());
    if (hr_read_accumulator(ctxs[0], sum_acc.data()) != 0) return 1;
    for (uint32_t r = 1; r < ndev; r++) {
        if (hr_read_accumulator(ctxs[r], part.data()) != 0) return 1;
        for (size_t i = 0; i < sum_acc.size(); i++) sum_acc[i] += part[i];
    }
    return 0;
}
// host-side sum: device 0 resolves the total from its accumulator, then gets its own partial sums back
int Run::resolve(uint32_t s, uint8_t *out) {
    if (o.robust_k) {   // (one device, no --denoise: checked with the flags)
        bool denoised = false;
        if (o.robust_denoise && final_image) {
            hr_denoise_params dp;
            if (hr_denoise_default_params(&dp) != 0) return 1;
            if (o.denoise_levels >= 0) dp.levels = (uint32_t)o.denoise_levels;
            const int rc = hr_denoise_robust(ctx, &dp);   // (HR_ERR_INVALID: a pixel with fewer than K samplings — the flags' values were checked when they were read)
            if (rc == 0) { have_guides = true; denoised = true; if (!o.robust_restore) return hr_resolve_denoised(ctx, out); }   // (it rendered the guide planes, nothing has dropped them since)
            else if (rc != HR_ERR_INVALID) return rc;
            else tee("robust-denoise: fewer than K samplings behind a pixel, the robust image is not denoised.");
        }
        if (o.robust_restore && final_image) {   // on top of D when there is one, else of the robust radiance
            hr_restore_params rp;
            if (hr_restore_default_params(&rp) != 0) return 1;
            if (o.restore_levels >= 0) rp.levels = (uint32_t)o.restore_levels;
            rp.base = denoised ? 1u : 0u;
            const int rc = hr_robust_restore(ctx, &rp);   // (HR_ERR_INVALID: a pixel with fewer than K samplings)
            if (rc == 0) { have_guides = true; return hr_resolve_restored(ctx, out); }
            if (rc != HR_ERR_INVALID) return rc;
            tee("robust-restore: fewer than K samplings behind a pixel, the robust image is not restored.");
        }
        return hr_robust(ctx) != 0 ? 1 : hr_resolve_robust(ctx, out);
    }
    if (o.auto_k && final_image) {   // (one device, neither --robust nor --denoise: checked with the flags)
        hr_denoise_params dp;
        hr_select_params sp;
        if (select_params(&dp, &sp)) return 1;
        const int rc = hr_denoise_select(ctx, &dp, &sp);   // (HR_ERR_INVALID: a pixel with fewer than 2 samplings, or buckets that do not cover the moments' samplings)
        if (rc == 0) { have_guides = true; have_levels = true; select_levels = dp.levels; return hr_resolve_selected(ctx, out); }
        if (rc != HR_ERR_INVALID) return rc;
        tee("denoise-auto: %s; the image is not denoised.", hr_last_error());
    }
    if (o.denoise && final_image) {
        hr_denoise_params dp;
        if (hr_denoise_default_params(&dp) != 0) return 1;
        if (o.denoise_levels >= 0) dp.levels = (uint32_t)o.denoise_levels;
        const int rc = hr_denoise(ctx, &dp);   // (HR_ERR_INVALID: a pixel with fewer than 2 samplings — the flags' values were checked when they were read)
        if (rc == 0) { have_guides = true; return hr_resolve_denoised(ctx, out); }   // (hr_denoise rendered the guide planes, nothing has dropped them since)
        if (rc != HR_ERR_INVALID) return rc;
        tee("denoise: fewer than 2 samplings behind a pixel, the image is not denoised.");
    }
    if (o.have_adaptive) return hr_resolve_counted(ctx, out);   // every pixel with its own count (one device: checked with the flags)
    if (!host_sum) return hr_resolve(ctx, s, out);
    if (hr_read_accumulator(ctx, part.data()) != 0 || hr_write_accumulator(ctx, sum_acc.data()) != 0) return 1;
    int rc = hr_resolve(ctx, s, out);
    return hr_write_accumulator(ctx, part.data()) != 0 ? 1 : rc;
}

// --denoise-auto's parameters as the flags give them: hr_denoise_select's and, with --auto-noise, the estimate's of the image it will make
int Run::select_params(hr_denoise_params *dp, hr_select_params *sp) {
    if (hr_denoise_default_params(dp) != 0 || hr_select_default_params(sp) != 0) return 1;
    if (o.denoise_levels >= 0) dp->levels = (uint32_t)o.denoise_levels;
    if (o.select_smooth >= 0) sp->smooth = (uint32_t)o.select_smooth;
    return 0;
}
// The noise estimate of everything rendered so far.  Several devices: every device holds the moments of its own samplings; they are
// additive, so the host adds them in rank order (as sum_acc does for accumulators without RCCL), device 0 estimates the total and gets
// its own moments back.  tot_out / n_out: the summed moments and their count as well (for the checkpoint).
// Returns 0, 1 = error, 2 = fewer than two samplings behind the moments (no variance yet).
// --robust-noise (one device): the same questions asked of the sample buckets, e_R in place of e; 2 = a pixel with fewer than K samplings.
// --auto-noise (one device): asked of the image --denoise-auto shows, e_S in place of e; 2 = a pixel with fewer than 2 samplings.
int Run::noise_query(hr_noise *est, double *img, std::vector<double> *tot_out, uint64_t *n_out) {
    uint64_t n_own = 0, n_tot = 0;
    const size_t len = (size_t)o.out_w * o.out_h * 6;
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
    // (HR_ERR_INVALID: n < 2, with --robust-noise n < K — floor and threshold were checked with the flags)
    int rc;
    if (o.auto_noise) {
        hr_denoise_params dp;
        hr_select_params sp;
        if (select_params(&dp, &sp)) return 1;
        rc = hr_selected_noise_estimate(ctx, &dp, &sp, o.noise_floor, o.noise_e, est);
        if (rc == 0 && img) rc = hr_read_selected_noise_image(ctx, &dp, &sp, o.noise_floor, img);
    } else {
        rc = o.robust_noise ? hr_robust_noise_estimate(ctx, o.noise_floor, o.noise_e, est) : hr_noise_estimate(ctx, o.noise_floor, o.noise_e, est);
        if (rc == 0 && img) rc = o.robust_noise ? hr_read_robust_noise_image(ctx, o.noise_floor, img) : hr_read_noise_image(ctx, o.noise_floor, img);
    }
    if (ndev > 1 && hr_write_moments(ctx, mom_own.data(), n_own) != 0) return 1;
    if (tot_out) *tot_out = mom_tot;
    if (n_out) *n_out = n_tot;
    return rc == 0 ? 0 : (rc == HR_ERR_INVALID ? 2 : 1);
}
// one "noise:" line per check, after the "rendering:" lines of the samplings it covers
int Run::noise_check_now() {
    int rc = noise_query(&noise_last, nullptr, nullptr, nullptr);
    if (rc == 1) { fprintf(stderr, "hr_noise_estimate: %s\n", hr_last_error()); return 1; }
    noise_known = rc == 0;
    if (noise_known) printf("noise: samplings=%llu mean=%.9g max=%.9g above=%llu\n", (unsigned long long)noise_last.samplings, noise_last.mean_error, noise_last.max_error,
                            (unsigned long long)noise_last.pixels_above);
    return 0;
}
int Run::save(uint32_t s) {
    char path[32];
    snprintf(path, sizeof path, "%03u.png", counter);
    double t0 = now_sec();
    if (combine() || resolve(s, rgb.data()) != 0) { fprintf(stderr, "hr_resolve: %s\n", hr_last_error()); return 1; }
    printf("update_imgbuf: %.3f sec\n", now_sec() - t0);
    last_png = path;
    return hh_write_png_rgb8(path, rgb.data(), o.out_w, o.out_h);
}

// --resume: what this render demands of the file, and what it says when the file falls short (the sections themselves: checkpoint.h)
int Run::resume() {
    if (o.ckpt_in.empty()) return 0;
    const char *path = o.ckpt_in.c_str();
    const ckpt::File c = ckpt::read(path);
    bool ok = c.magic == ckpt::FRAME || c.magic == ckpt::REGION;
    if (ok && (c.magic == ckpt::REGION) != o.has_region) {
        fprintf(stderr, "cannot resume from %s: %s\n", path, o.has_region ? "it is a full-frame checkpoint and --region is given" : "it is a region checkpoint and no --region is given");
        return 1;
    }
    if (ok && o.has_region) {
        ok = c.complete >= ckpt::S_HEADER;
        if (ok && (c.region[0] != o.region[0] || c.region[1] != o.region[1] || c.region[2] != o.out_w || c.region[3] != o.out_h)) {
            fprintf(stderr, "cannot resume from %s: its region is %u,%u,%u,%u, --region is %u,%u,%u,%u\n", path, c.region[0], c.region[1], c.region[2], c.region[3],
                    o.region[0], o.region[1], o.out_w, o.out_h);
            return 1;
        }
    }
    ok = ok && c.width == o.width && c.height == o.height && c.scene_hash == scene_hash && c.complete >= ckpt::S_ACCUMULATOR;
    // The trailers count only for a render that keeps what they hold; a trailer that is cut short hides whatever is behind it.
    const bool have_mom = c.has_moments && o.moments;   // (moments that are cut short: as a file without them)
    const uint64_t mom_n = c.moments_n;
    std::vector<uint32_t> uniform;
    if (ok && o.counts) {
        // a file without counts was rendered uniformly: every pixel has received all of its samplings
        resumed_counts = c.has_counts;
        if (!resumed_counts) uniform.assign((size_t)o.out_w * o.out_h, c.samplings);
        ok = c.cut != ckpt::S_COUNTS;
    }
    const char *bkt_why = nullptr;
    if (ok && o.robust_k) {
        if (!o.counts && (c.has_counts || c.cut == ckpt::S_COUNTS)) bkt_why = "its buckets were filled by per-pixel sampling counts (resume with --adaptive or --sample-image as well)";
        else if (!c.buckets_head) bkt_why = "it holds no sample buckets (it was written without --robust)";
        else if (c.buckets_k != (uint32_t)o.robust_k) bkt_why = "its sample buckets were kept with another K";
        else ok = c.has_buckets;
    }
    if (!ok) { fprintf(stderr, "cannot resume from %s (missing, wrong magic, resolution or scene)\n", path); return 1; }
    if (bkt_why) {
        fprintf(stderr, "--resume %s with --robust %lld: %s; resume without --robust, or render again with it.\n", path, o.robust_k, bkt_why);
        return 1;
    }
    if (o.have_adaptive && !have_mom) {
        fprintf(stderr, "--resume %s with --adaptive: the checkpoint holds no sample moments (it was written without --adaptive / --noise-target / --noise-image), "
                        "so the noise of its %u samplings cannot be known; resume without --adaptive, or render again with it.\n", path, c.samplings);
        return 1;
    }
    if (o.have_adaptive && !resumed_counts && mom_n != c.samplings) {
        fprintf(stderr, "--resume %s with --adaptive: its sample moments cover %llu of its %u samplings and it holds no per-pixel counts, "
                        "so the noise of its pixels cannot be known; resume without --adaptive, or render again with it.\n", path, (unsigned long long)mom_n, c.samplings);
        return 1;
    }
    if (o.denoise && !(have_mom && (resumed_counts || mom_n == c.samplings))) {
        // the filter's mean is accumulator / (4 n) with n the samplings behind the moments (or the pixel's count): moments that do not cover
        // every sampling of the accumulator would give an image of the wrong brightness
        fprintf(stderr, "--resume %s with --denoise: the checkpoint's sample moments %s, so the variance of its %u samplings cannot be known; "
                        "resume without --denoise, or render again with it.\n", path,
                have_mom ? "do not cover all of its samplings" : "are missing (it was written without --denoise / --adaptive / --noise-target / --noise-image)", c.samplings);
        return 1;
    }
    if (o.have_target && !have_mom) {
        fprintf(stderr, "--resume %s with --noise-target: the checkpoint holds no sample moments (it was written without --noise-target / --noise-image), "
                        "so the noise of its %u samplings cannot be known; resume without --noise-target, or render again with it.\n", path, c.samplings);
        return 1;
    }
    CHECK_HR(hr_write_accumulator(ctx, c.acc.data()));
    if (o.counts) CHECK_HR(hr_write_sample_counts(ctx, resumed_counts ? c.counts.data() : uniform.data()));
    if (have_mom) CHECK_HR(hr_write_moments(ctx, c.moments.data(), mom_n));
    else if (o.moments) printf("the checkpoint holds no sample moments: the noise image covers the samplings rendered from here on\n");
    if (o.robust_k) CHECK_HR(hr_write_buckets(ctx, c.buckets.data(), c.buckets_n));
    first = c.samplings + 1;
    sampled = c.samplings;
    printf("resumed at %ux4 sampled\n", c.samplings);
    return 0;
}

int Run::render() {
    const bool debug = o.debug, have_target = o.have_target, have_adaptive = o.have_adaptive;
    const double time_limit = o.time_limit, interval = o.interval, noise_floor = o.noise_floor, noise_target = o.noise_target, adaptive_e = o.adaptive_e;
    const uint32_t out_w = o.out_w, out_h = o.out_h;
    const long long noise_check = o.noise_check;
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
    const uint32_t B = (uint32_t)o.batch;
    uint32_t lrep = o.launch > 0 ? (uint32_t)o.launch : 0;   // reports per launch
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
    const size_t depth = interval <= 0.0 ? 1 : (size_t)o.inflight;
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
            // (HR_ERR_INVALID: a pixel with fewer than 2 samplings, with --robust-noise fewer than K — no estimate yet, go on as before)
            int rc;
            if (o.auto_noise) {   // (--auto-noise: e_S of the image --denoise-auto will show)
                hr_denoise_params dp;
                hr_select_params sp;
                if (select_params(&dp, &sp)) return 1;
                rc = hr_select_tiles_selected(ctx, &dp, &sp, noise_floor, adaptive_e, &active);
            } else rc = o.robust_noise ? hr_select_tiles_robust(ctx, noise_floor, adaptive_e, &active) : hr_select_tiles(ctx, noise_floor, adaptive_e, &active);
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
    return 0;
}

// the whole camera — eye and all five vectors — turned by `degrees` about the vertical axis through eye + focus_distance x forward
static hr_camera orbit_camera(const hr_camera &c, double degrees) {
    const double a = degrees * 3.14159265358979323846 / 180.0, ca = cos(a), sa = sin(a);
    auto rot = [&](const hr_vec3 &v) { return hr_vec3{ca * v.x + sa * v.z, v.y, ca * v.z - sa * v.x}; };
    const hr_vec3 pivot = {c.eye.x + c.focus_distance * c.forward.x, c.eye.y + c.focus_distance * c.forward.y, c.eye.z + c.focus_distance * c.forward.z};
    hr_camera out = c;
    const hr_vec3 rel = rot(hr_vec3{c.eye.x - pivot.x, c.eye.y - pivot.y, c.eye.z - pivot.z});
    out.eye = hr_vec3{pivot.x + rel.x, pivot.y + rel.y, pivot.z + rel.z};
    out.right = rot(c.right); out.up = rot(c.up); out.forward = rot(c.forward);
    out.plane_half_right = rot(c.plane_half_right); out.plane_half_up = rot(c.plane_half_up);
    return out;
}
// --frames N: frame f is samplings f S + 1 .. (f + 1) S at the camera of frame f - 1 turned by --orbit, set with hr_set_camera (the scene and its tree
// stay).  With --temporal M it starts from frame f - 1's accumulator, counts and moments, reprojected (hr_render_motion of the previous camera,
// hr_reproject); without, from nothing.  Every frame is resolved with the pixels' own counts, with --denoise through hr_denoise.  The samplings go out
// in the launches Run::render makes of them, so --frames 1 writes the plain run's final image.
int Run::render_frames() {
    const uint32_t S = o.sampling;
    const uint64_t per_sampling = ((uint64_t)(o.out_w + 3) / 4) * ((o.out_h + 3) / 4) * 64u;
    const uint32_t lsize = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(4, (33177600ull + per_sampling - 1) / per_sampling));
    hr_camera cam, prev;
    CHECK_HR(hr_get_camera(ctx, &cam));
    hr_reproject_params rp;
    CHECK_HR(hr_reproject_default_params(&rp));
    if (o.temporal) rp.max_history = (uint32_t)o.temporal;
    std::vector<uint32_t> counts((size_t)o.out_w * o.out_h);
    for (uint32_t f = 0; f < (uint32_t)o.frames; f++) {
        const double t0 = now_sec();
        uint32_t history = 0;
        if (f) {
            prev = cam;
            cam = orbit_camera(prev, o.orbit_deg);
            CHECK_HR(hr_set_camera(ctx, &cam));
            if (o.temporal) {
                CHECK_HR(hr_render_motion(ctx, &prev, &rp));
                CHECK_HR(hr_reproject(ctx, &rp));
                CHECK_HR(hr_read_sample_counts(ctx, counts.data()));
                for (uint32_t n : counts) history = std::max(history, n);
            } else CHECK_HR(hr_clear(ctx));
        }
        const uint32_t begin_s = f * S + 1, end_s = begin_s + S;
        for (uint32_t b = begin_s; b < end_s; b += lsize) CHECK_HR(hr_render(ctx, b, std::min(end_s, b + lsize), 1));
        CHECK_HR(hr_synchronize(ctx));
        final_image = true;
        sampled = end_s - 1;
        bool denoised = false;
        if (o.denoise) {
            hr_denoise_params dp;
            CHECK_HR(hr_denoise_default_params(&dp));
            if (o.denoise_levels >= 0) dp.levels = (uint32_t)o.denoise_levels;
            const int rc = hr_denoise(ctx, &dp);   // (HR_ERR_INVALID: a pixel with fewer than 2 samplings)
            if (rc == 0) { CHECK_HR(hr_resolve_denoised(ctx, rgb.data())); denoised = true; }
            else if (rc != HR_ERR_INVALID) { fprintf(stderr, "hr_denoise: %s\n", hr_last_error()); return 1; }
            else tee("denoise: fewer than 2 samplings behind a pixel, frame %u is not denoised.", f);
        }
        if (!denoised) CHECK_HR(hr_resolve_counted(ctx, rgb.data()));
        char path[32];
        snprintf(path, sizeof path, "frame_%03u.png", f);
        if (write_png(path, rgb.data(), o.out_w, o.out_h)) return 1;
        tee("frame %u: samplings %u .. %u, history up to %u, %s, %.3f sec.", f, begin_s, end_s - 1, history, path, now_sec() - t0);
    }
    return 0;
}

// --checkpoint: everything is read from the devices first, then written in one go; a file keeps the bytes it always had: the trailers
// of what this render did not keep are not there
int Run::write_checkpoint() {
    if (o.ckpt_out.empty()) return 0;
    ckpt::File c;
    c.magic = o.has_region ? ckpt::REGION : ckpt::FRAME, c.width = o.width, c.height = o.height, c.samplings = sampled, c.scene_hash = scene_hash;
    std::copy(o.region, o.region + 4, c.region);
    c.has_moments = o.moments, c.has_counts = o.counts, c.has_buckets = o.robust_k != 0;
    c.acc.resize((size_t)o.out_w * o.out_h * 3);
    if (combine()) { fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
    if (host_sum) c.acc = sum_acc;
    else CHECK_HR(hr_read_accumulator(ctx, c.acc.data()));
    if (c.has_moments) {
        hr_noise est;
        if (noise_query(&est, nullptr, &c.moments, &c.moments_n) == 1) { fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
    }
    if (c.has_counts) {
        c.counts.resize((size_t)o.out_w * o.out_h);
        if (hr_read_sample_counts(ctx, c.counts.data()) != 0) { fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
    }
    if (c.has_buckets) {
        c.buckets_k = (uint32_t)o.robust_k;
        c.buckets.resize((size_t)o.out_w * o.out_h * 3 * c.buckets_k);
        if (hr_read_buckets(ctx, c.buckets.data(), &c.buckets_n) != 0) { fprintf(stderr, "checkpoint: %s\n", hr_last_error()); return 1; }
    }
    if (!ckpt::write(o.ckpt_out.c_str(), c)) { fprintf(stderr, "cannot write checkpoint %s\n", o.ckpt_out.c_str()); return 1; }
    return 0;
}

// main.rs:1217: result.png = the final image — the bytes finish() has just written as NNN.png
int Run::write_result_png() {
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
    return copied ? 0 : write_png("result.png", rgb.data(), o.out_w, o.out_h);
}

// what the render came to, to result.txt as well, and the maps of it that were asked for
int Run::write_reports() {
    const uint32_t out_w = o.out_w, out_h = o.out_h;
    const size_t pixels = (size_t)out_w * out_h;
    if (o.moments) {   // the estimate of the final image; and its map
        std::vector<double> e_img(o.noise_png.empty() ? 0 : pixels);
        int rc = noise_query(&noise_last, e_img.empty() ? nullptr : e_img.data(), nullptr, nullptr);
        if (rc == 1) { fprintf(stderr, "hr_noise_estimate: %s\n", hr_last_error()); return 1; }
        if (rc == 2) tee("noise: fewer than 2 samplings, no estimate.");
        else tee("noise: samplings=%llu mean=%.9g max=%.9g above=%llu", (unsigned long long)noise_last.samplings, noise_last.mean_error, noise_last.max_error,
                 (unsigned long long)noise_last.pixels_above);
        const double E = o.noise_e > 0.0 ? o.noise_e : 0.05;   // grey map of min(1, e / E)
        if (!o.noise_png.empty() && rc == 0 && write_grey(o.noise_png, out_w, out_h, [&](size_t i) { const double t = e_img[i] / E; return t >= 1.0 ? 1.0 : (t > 0.0 ? t : 0.0); })) return 1;
    }
    if (!o.guide_prefix.empty()) {   // the guide planes as images of their own (the planes of --denoise's filter, or a pass of their own)
        std::vector<float> g(pixels * 8);
        if (!have_guides) CHECK_HR(hr_render_guides(ctx));
        CHECK_HR(hr_read_guides(ctx, g.data()));
        float zmax = 0.0f;
        for (size_t i = 0; i < pixels; i++) zmax = std::max(zmax, g[i * 8 + 6]);
        auto byte = [](float v) { return (uint8_t)(std::min(1.0f, std::max(0.0f, v)) * 255.0f + 0.5f); };
        std::vector<uint8_t> img(pixels * 3);
        for (size_t i = 0; i < pixels; i++) for (int k = 0; k < 3; k++) img[i * 3 + k] = byte(powf(std::max(0.0f, g[i * 8 + k]), 1.0f / 2.2f));
        if (write_png(o.guide_prefix + "_albedo.png", img.data(), out_w, out_h)) return 1;
        for (size_t i = 0; i < pixels; i++) for (int k = 0; k < 3; k++) img[i * 3 + k] = byte(0.5f * g[i * 8 + 3 + k] + 0.5f * g[i * 8 + 7]);
        if (write_png(o.guide_prefix + "_normal.png", img.data(), out_w, out_h)) return 1;
        if (write_grey(o.guide_prefix + "_depth.png", out_w, out_h, [&](size_t i) { return std::min(1.0f, std::max(0.0f, zmax > 0.0f ? g[i * 8 + 6] / zmax : 0.0f)); })) return 1;
    }
    if (o.auto_k && have_levels) {   // which level the pixels took; and its map
        std::vector<uint8_t> lev(pixels);
        CHECK_HR(hr_read_selected_levels(ctx, lev.data()));
        uint64_t sum = 0;
        for (uint8_t v : lev) sum += v;
        tee("denoise-auto: buckets=%lld levels=%u mean level=%.3f", o.auto_k, select_levels, (double)sum / (double)lev.size());
        // grey map of level / levels
        if (!o.level_png.empty() && write_grey(o.level_png, out_w, out_h, [&](size_t i) { return select_levels ? (double)lev[i] / (double)select_levels : 0.0; })) return 1;
    }
    if (o.robust_k) {   // how much the robust resolve dropped; and its map
        std::vector<uint8_t> trim(pixels);
        CHECK_HR(hr_robust(ctx));
        CHECK_HR(hr_read_robust_trim(ctx, trim.data()));
        const uint32_t most = (uint32_t)(o.robust_k - 1) / 2;
        size_t trimmed = 0;
        for (uint8_t v : trim) trimmed += v != 0;
        tee("robust: buckets=%lld trimmed pixels=%.4f", o.robust_k, (double)trimmed / (double)trim.size());
        // grey map of trim / ((K - 1) / 2)
        if (!o.robust_png.empty() && write_grey(o.robust_png, out_w, out_h, [&](size_t i) { return (double)trim[i] / (double)most; })) return 1;
    }
    if (o.counts) {   // how the samplings were spent
        std::vector<uint32_t> cnt(pixels);
        CHECK_HR(hr_read_sample_counts(ctx, cnt.data()));
        uint32_t lo = ~0u, hi = 0;
        uint64_t sum = 0;
        for (uint32_t v : cnt) { lo = std::min(lo, v); hi = std::max(hi, v); sum += v; }
        tee("samplings per pixel: min=%u max=%u mean=%.3f", lo, hi, (double)sum / (double)cnt.size());
        // grey map of count / largest count
        if (!o.sample_png.empty() && write_grey(o.sample_png, out_w, out_h, [&](size_t i) { return hi ? (double)cnt[i] / (double)hi : 0.0; })) return 1;
    }
    tee("sampled: %ux%u spp.", sampled, 4u);
    hr_stats st;
    if (hr_get_stats(ctx, &st) == 0) {
        double sec = st.trace_kernel_ms * 1e-3;
        uint64_t paths = st.paths;
        for (uint32_t r = 1; r < ndev; r++) { hr_stats other; if (hr_get_stats(ctxs[r], &other) == 0) paths += other.paths; }
        // two clocks: until the last sampling was reported (the render itself), and until here (+ the final hr_resolve and the PNG encoder)
        tee("gpu: %.3f Mpaths/s wall (%.3f incl. the final image), trace kernel %.3f s, seed kernel %.3f s.", (double)paths / std::max(1e-9, last_progress - begin) * 1e-6,
            (double)paths / (now_sec() - begin) * 1e-6, sec, st.seed_kernel_ms * 1e-3);
    }
    double total = now_sec() - total_begin;
    double used_percent = total / o.time_limit * 100.0;
    tee("total %g sec. used %.2f %% (x %.2f)", total, used_percent, 100.0 / used_percent);
    return 0;
}

void Run::close() {
    for (hr_ctx *c : ctxs) hr_destroy(c);
    hh_scene_destroy(scene);
    if (g_log) fclose(g_log);
}

int main(int argc, char **argv) {
    Options o;
    const int status = parse_options(argc, argv, o);
    if (status >= 0) return status;
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);   // dmabuf IPC (RCCL on this driver), unless the caller says otherwise; before the HIP runtime starts
    g_log = fopen("result.txt", "w");
    Run run(o);
    run.print_settings();
    if (o.frames) {
        if (run.open_devices() || run.render_frames()) return 1;
    } else if (run.open_devices() || run.resume() || run.render() || run.write_checkpoint() || run.write_result_png() || run.write_reports()) return 1;
    run.close();
    return 0;
}
