// cli.cpp — `maray` command line (product code).  Mirrors examples/maray.rs:
//   maray -c N -i in.maray -o out.png [-t tex.png ...]        (:9-47)
// plus --gpus N, --backend {tape,tape-smem,jit}, -s/--samples k (anti-aliasing), --filter {box,tent,catrom} (how the samples become
// pixels), -p NAME=VALUE[:LO:HI] (a scene parameter:
// the free variable `var(NAME)` gets VALUE at render time) and --animate NAME=FROM:TO:FRAMES (one image per value, all from
// the one program and the contexts the first frame set up), --shutter NAME=SPAN / --shutter-samples N (motion blur: every
// image the mean of N frames whose NAME covers SPAN around its value, averaged on the device), --linear (samples and frames
// are averaged in linear light: include/maray_hip.h, "transfer"), --encoder {host,device} (who
// writes the PNG: the host's zlib, or the device encoder, per --animate frame too), --apng (--animate writes ONE file, an APNG
// encoded on the device frame by frame: include/maray_hip.h, "animation"; --fps N[/D] and --loops N are its timing), --y4m
// (--animate writes ONE file, a YUV4MPEG2 video whose Y'CbCr planes are converted on the device: include/maray_hip.h, "raw
// video"; --y4m-sampling and --y4m-matrix choose the planes, --fps the rate).
// -c/--cpus is parsed and ignored, exactly like the reference (`_cpus`, examples/maray.rs:55).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "maray_hip.h"

static void usage()
{
    fprintf(stderr,
            "Maray 0.3 (MI355X)\nJIT Ray Tracing using basic math\n\n"
            "Usage: maray [OPTIONS] --input <input> --output <output>\n\n"
            "  -c, --cpus <cpus>            Number of CPU cores (accepted, unused)\n"
            "  -i, --input <input>          Input file `*.maray`\n"
            "  -o, --output <output>        Output file `*.png`\n"
            "  -t, --textures <textures>... Texture files (PNG, BMP, PNM, TGA, QOI, farbfeld, GIF, TIFF)\n"
            "      --gpus <n>               Number of MI355X devices (default: all)\n"
            "      --backend <b>            auto | jit | tape | tape-smem (default: auto)\n"
            "  -s, --samples <k>            Anti-aliasing: k x k samples per pixel, box-filtered; k = 1, 2, 4 or 8 (default: 1)\n"
            "      --filter <f>             box | tent | catrom (default: box); tent is two pixels wide, catrom (Catmull-Rom) four\n"
            "                               with negative lobes; both need -s 2, 4 or 8, and catrom does not go with --linear\n"
            "  -p, --param <name=v[:lo:hi]> Value of the scene's free variable `name` (repeatable); lo:hi = the range it is\n"
            "                               declared with (default: any value)\n"
            "      --animate <name=a:b:n>   n images, `name` going from a to b in equal steps; --output needs a `%%d`\n"
            "                               conversion (`frame%%03d.png`), numbered from 0\n"
            "      --apng                   With --animate: one file, an animated PNG (APNG) whose frames are encoded on the GPU, of\n"
            "                               every frame after the first only the rectangle that changed; --output takes no `%%d`,\n"
            "                               --gpus must be 1 or absent\n"
            "      --y4m                    With --animate: one file, a YUV4MPEG2 video (what ffmpeg, x264, SVT-AV1 and aomenc read):\n"
            "                               limited-range Y'CbCr planes converted on the GPU; --output takes no `%%d`, --gpus must be\n"
            "                               1 or absent, not together with --apng\n"
            "      --y4m-sampling <s>       --y4m: 420 | 444 (default: 420, chroma sited as in JPEG)\n"
            "      --y4m-matrix <m>         --y4m: 601 | 709 (default: 601); the file has no tag for it: tell the encoder\n"
            "      --fps <n[/d]>            --apng, --y4m: n / d images per second (default: 25)\n"
            "      --loops <n>              --apng: how often the animation plays; 0 = for ever (default: 0)\n"
            "      --shutter <name=span>    Motion blur (repeatable): every image is the mean of N frames in which `name` covers\n"
            "                               an interval of width span centred on its value; declares `name` if -p did not\n"
            "      --shutter-samples <n>    N = 1, 2, 4, 8, 16, 32 or 64 (default: 8 once a --shutter is given)\n"
            "      --linear                 Average samples (-s) and shutter frames in linear light: bytes are decoded as sRGB,\n"
            "                               averaged and encoded again; alone it changes nothing\n"
            "      --encoder <e>            host | device (default: host); device builds the PNG's compressed stream on the GPU,\n"
            "                               so that no raster crosses to the host (same pixels, other file bytes)\n"
            "      --png-codes <c>          fixed | dynamic (default: fixed); needs --encoder device or --apng.  dynamic fits a Huffman\n"
            "                               code to every band of rows: the same pixels in a several times smaller file\n");
}

namespace {
struct Param { std::string name; double value, lo, hi; };

// "a:b:c" -> numbers, every field a whole strtod
bool numbers(const std::string &t, std::vector<double> &out)
{
    size_t at = 0;
    for (;;) {
        const size_t end = t.find(':', at);
        const std::string f = t.substr(at, end == std::string::npos ? std::string::npos : end - at);
        char *rest = nullptr;
        const double v = strtod(f.c_str(), &rest);
        if (f.empty() || !rest || *rest) return false;
        out.push_back(v);
        if (end == std::string::npos) return true;
        at = end + 1;
    }
}

bool split_name(const std::string &arg, std::string &name, std::vector<double> &nums)
{
    const size_t eq = arg.find('=');
    if (eq == std::string::npos || eq == 0) return false;
    name = arg.substr(0, eq);
    return numbers(arg.substr(eq + 1), nums);
}

// exactly one conversion, %d with an optional zero-padded width
bool numbered(const std::string &path)
{
    const size_t at = path.find('%');
    if (at == std::string::npos || path.find('%', at + 1) != std::string::npos) return false;
    size_t k = at + 1;
    while (k < path.size() && path[k] >= '0' && path[k] <= '9') k++;
    return k < path.size() && path[k] == 'd' && k - at <= 4;
}
}   // namespace

int main(int argc, char **argv)
{
    std::string input, output;
    std::vector<std::string> textures;
    std::vector<Param> params;
    Param anim; uint32_t frames = 0;
    std::vector<Param> spans;           // --shutter: name, value = the span
    uint32_t shutter_samples = 0;
    bool linear = false;                // --linear
    bool apng = false;                  // --apng
    bool y4m = false, y4m_words = false;                // --y4m; a --y4m-sampling or --y4m-matrix was given
    maray_anim_opts ao;
    memset(&ao, 0, sizeof ao);
    bool png_codes_given = false, dynamic_codes = false;      // --png-codes
    uint32_t fps_num = 25, fps_den = 1, loops = 0;
    maray_gen_opts go;
    memset(&go, 0, sizeof go);
    go.backend = MARAY_BACKEND_AUTO;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char * { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-c" || a == "--cpus") (void)strtoul(val(), nullptr, 10);
        else if (a == "-i" || a == "--input") input = val();
        else if (a == "-o" || a == "--output") output = val();
        else if (a == "-t" || a == "--textures") { while (i + 1 < argc && argv[i + 1][0] != '-') textures.push_back(argv[++i]); }
        else if (a == "--gpus") go.n_devices = (uint32_t)strtoul(val(), nullptr, 10);
        else if (a == "-s" || a == "--samples") {
            const std::string k = val();
            if (k != "1" && k != "2" && k != "4" && k != "8") {
                fprintf(stderr, "Error: --samples takes 1, 2, 4 or 8, not `%s`\n", k.c_str());
                usage();
                return 2;
            }
            go.samples = (uint32_t)(k[0] - '0');
        }
        else if (a == "--filter") {
            const std::string f = val();
            if (f == "box") go.filter = MARAY_FILTER_BOX;
            else if (f == "tent") go.filter = MARAY_FILTER_TENT;
            else if (f == "catrom") go.filter = MARAY_FILTER_CATROM;
            else { fprintf(stderr, "Error: --filter takes box, tent or catrom, not `%s`\n", f.c_str()); usage(); return 2; }
        }
        else if (a == "--linear") linear = true;
        else if (a == "--apng") apng = true;
        else if (a == "--y4m") y4m = true;
        else if (a == "--y4m-sampling") {
            const std::string e = val();
            y4m_words = true;
            if (e == "420") ao.sampling = MARAY_YCC_420;
            else if (e == "444") ao.sampling = MARAY_YCC_444;
            else { fprintf(stderr, "Error: --y4m-sampling takes 420 or 444, not `%s`\n", e.c_str()); usage(); return 2; }
        }
        else if (a == "--y4m-matrix") {
            const std::string e = val();
            y4m_words = true;
            if (e == "601") ao.matrix = MARAY_YCC_BT601;
            else if (e == "709") ao.matrix = MARAY_YCC_BT709;
            else { fprintf(stderr, "Error: --y4m-matrix takes 601 or 709, not `%s`\n", e.c_str()); usage(); return 2; }
        }
        else if (a == "--fps") {
            const std::string f = val();
            char *rest = nullptr;
            const unsigned long n = strtoul(f.c_str(), &rest, 10);
            unsigned long d = 1;
            bool ok = !f.empty() && f[0] >= '0' && f[0] <= '9' && rest && (*rest == 0 || *rest == '/');
            if (ok && *rest == '/') {
                const char *t = rest + 1;
                ok = *t >= '0' && *t <= '9';
                d = strtoul(t, &rest, 10);
                ok = ok && rest && !*rest;
            }
            if (!ok || n < 1 || n > 65535 || d < 1 || d > 65535) { fprintf(stderr, "Error: --fps takes N or N/D with N and D in 1 .. 65535, not `%s`\n", f.c_str()); usage(); return 2; }
            fps_num = (uint32_t)n; fps_den = (uint32_t)d;
        }
        else if (a == "--loops") {
            const std::string f = val();
            char *rest = nullptr;
            const unsigned long n = strtoul(f.c_str(), &rest, 10);
            if (f.empty() || f[0] < '0' || f[0] > '9' || !rest || *rest || n > 0xFFFFFFFFul) { fprintf(stderr, "Error: --loops takes a count >= 0, not `%s`\n", f.c_str()); usage(); return 2; }
            loops = (uint32_t)n;
        }
        else if (a == "--encoder") {
            const std::string e = val();
            if (e == "host") go.encoder = MARAY_ENCODER_HOST;
            else if (e == "device") go.encoder = MARAY_ENCODER_DEVICE;
            else { fprintf(stderr, "Error: --encoder takes host or device, not `%s`\n", e.c_str()); usage(); return 2; }
        }
        else if (a == "--png-codes") {
            const std::string e = val();
            png_codes_given = true;
            if (e == "fixed") dynamic_codes = false;
            else if (e == "dynamic") dynamic_codes = true;
            else { fprintf(stderr, "Error: --png-codes takes fixed or dynamic, not `%s`\n", e.c_str()); usage(); return 2; }
        }
        else if (a == "-p" || a == "--param") {
            Param p; std::vector<double> n;
            if (!split_name(val(), p.name, n) || (n.size() != 1 && n.size() != 3)) { fprintf(stderr, "Error: -p takes NAME=VALUE or NAME=VALUE:LO:HI\n"); usage(); return 2; }
            p.value = n[0]; p.lo = n.size() == 3 ? n[1] : -INFINITY; p.hi = n.size() == 3 ? n[2] : INFINITY;
            params.push_back(p);
        }
        else if (a == "--animate") {
            std::vector<double> n;
            if (!split_name(val(), anim.name, n) || n.size() != 3 || !(n[2] >= 1.0 && n[2] <= 1e6) || n[2] != std::floor(n[2]) || !(n[0] == n[0] && n[1] == n[1])) {
                fprintf(stderr, "Error: --animate takes NAME=FROM:TO:FRAMES with FRAMES >= 1\n"); usage(); return 2;
            }
            anim.value = n[0]; anim.hi = n[1]; frames = (uint32_t)n[2];
        }
        else if (a == "--shutter") {
            Param p; std::vector<double> n;
            if (!split_name(val(), p.name, n) || n.size() != 1 || !(n[0] >= 0.0) || !std::isfinite(n[0])) {
                fprintf(stderr, "Error: --shutter takes NAME=SPAN with a finite SPAN >= 0\n"); usage(); return 2;
            }
            p.value = n[0]; p.lo = p.hi = 0.0;
            spans.push_back(p);
        }
        else if (a == "--shutter-samples") {
            const std::string k = val();
            if (k != "1" && k != "2" && k != "4" && k != "8" && k != "16" && k != "32" && k != "64") {
                fprintf(stderr, "Error: --shutter-samples takes 1, 2, 4, 8, 16, 32 or 64, not `%s`\n", k.c_str());
                usage();
                return 2;
            }
            shutter_samples = (uint32_t)strtoul(k.c_str(), nullptr, 10);
        }
        else if (a == "--backend") {
            std::string b = val();
            if (b == "tape") go.backend = MARAY_BACKEND_TAPE;
            else if (b == "tape-smem") go.backend = MARAY_BACKEND_TAPE_SMEM;
            else if (b == "jit") go.backend = MARAY_BACKEND_JIT;
            else if (b == "auto") go.backend = MARAY_BACKEND_AUTO;
            else { usage(); return 2; }
        } else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { usage(); return 2; }
    }
    if (input.empty() || output.empty()) { usage(); return 2; }
    if (go.filter == MARAY_FILTER_TENT && go.samples < 2) { fprintf(stderr, "Error: --filter tent needs -s 2, 4 or 8\n"); usage(); return 2; }
    if (go.filter == MARAY_FILTER_CATROM && go.samples < 2) { fprintf(stderr, "Error: --filter catrom needs -s 2, 4 or 8\n"); usage(); return 2; }
    if (go.filter == MARAY_FILTER_CATROM && linear) {
        fprintf(stderr, "Error: --filter catrom does not go with --linear: the Catmull-Rom filter in linear light is not built\n");
        usage();
        return 2;
    }
    if (png_codes_given && go.encoder != MARAY_ENCODER_DEVICE && !apng) {
        fprintf(stderr, "Error: --png-codes chooses the device encoder's codes: it needs --encoder device or --apng\n");
        usage();
        return 2;
    }
    if (dynamic_codes) go.encoder |= MARAY_ENCODER_DYNAMIC;
    if (apng && !frames) { fprintf(stderr, "Error: --apng writes an animation: it needs --animate NAME=FROM:TO:FRAMES\n"); return 2; }
    if (apng && output.find('%') != std::string::npos) { fprintf(stderr, "Error: --apng writes one file: --output must not contain a `%%d` conversion\n"); return 2; }
    if (apng && go.n_devices > 1) { fprintf(stderr, "Error: --apng renders and encodes on one device: --gpus must be 1\n"); return 2; }
    if (y4m && apng) { fprintf(stderr, "Error: --y4m and --apng both write the animation as one file: choose one\n"); usage(); return 2; }
    if (y4m_words && !y4m) { fprintf(stderr, "Error: --y4m-sampling and --y4m-matrix choose the planes of a --y4m file: they need --y4m\n"); usage(); return 2; }
    if (y4m && !frames) { fprintf(stderr, "Error: --y4m writes an animation: it needs --animate NAME=FROM:TO:FRAMES\n"); usage(); return 2; }
    if (y4m && output.find('%') != std::string::npos) { fprintf(stderr, "Error: --y4m writes one file: --output must not contain a `%%d` conversion\n"); usage(); return 2; }
    if (y4m && go.n_devices > 1) { fprintf(stderr, "Error: --y4m renders and converts on one device: --gpus must be 1\n"); usage(); return 2; }
    const bool one_file = apng || y4m;
    if (frames && !one_file && !numbered(output)) { fprintf(stderr, "Error: --animate writes several images: --output needs one `%%d` conversion, e.g. frame%%03d.png\n"); return 2; }

    maray_scene *scene = nullptr;
    if (maray_scene_open(input.c_str(), &scene)) { fprintf(stderr, "Error: %s\n", maray_last_error()); return 1; }
    std::vector<maray_texture> tex;
    std::vector<uint8_t *> rasters;
    for (const std::string &t : textures) {
        uint8_t *rgb = nullptr; uint32_t w = 0, h = 0;
        if (maray_image_read(t.c_str(), &rgb, &w, &h)) { fprintf(stderr, "Error: %s: %s\n", t.c_str(), maray_last_error()); return 1; }
        rasters.push_back(rgb);
        tex.push_back(maray_texture{rgb, w, h});
    }
    // parameters: declared with their ranges and set; a value its range excludes is the command line's mistake
    for (const Param &p : params) {
        uint32_t k = 0;
        if (maray_scene_declare_param(scene, maray_var_id(p.name.c_str()), p.lo, p.hi, &k) || maray_scene_set_param(scene, k, p.value)) {
            fprintf(stderr, "Error: -p %s: %s\n", p.name.c_str(), maray_last_error());
            return 2;
        }
    }
    // --animate and --shutter declare what -p did not: --animate the range its frames need, [FROM, TO] widened by half the
    // name's span on both sides; --shutter alone any value, like -p.  A -p declaration stands as given: a frame outside an
    // explicit LO:HI is the command line's mistake.
    auto index_of = [&](const std::string &name, uint32_t &k) {
        uint32_t n_par = 0;
        maray_scene_param_count(scene, &n_par);
        const uint64_t want = maray_var_id(name.c_str());
        for (k = 0; k < n_par; k++) {
            uint64_t id = 0;
            maray_scene_param_info(scene, k, &id, nullptr, nullptr, nullptr);
            if (id == want) return true;
        }
        return false;
    };
    uint32_t anim_index = 0;
    const double from = anim.value, to = anim.hi;
    if (frames && !index_of(anim.name, anim_index)) {
        double half = 0.0;
        for (const Param &sp : spans) if (sp.name == anim.name) half = sp.value / 2;
        if (maray_scene_declare_param(scene, maray_var_id(anim.name.c_str()), std::fmin(from, to) - half, std::fmax(from, to) + half, &anim_index)) {
            fprintf(stderr, "Error: --animate %s: %s\n", anim.name.c_str(), maray_last_error());
            return 2;
        }
    }
    for (const Param &sp : spans) {
        uint32_t k = 0;
        if ((!index_of(sp.name, k) && maray_scene_declare_param(scene, maray_var_id(sp.name.c_str()), -INFINITY, INFINITY, &k)) ||
            maray_scene_set_param_span(scene, k, sp.value)) {
            fprintf(stderr, "Error: --shutter %s: %s\n", sp.name.c_str(), maray_last_error());
            return 2;
        }
    }
    if (!spans.empty()) go.shutter = shutter_samples ? shutter_samples : 8;
    // --linear alone has nothing to reduce: the plain render, from the plain render's program and contexts
    if (linear && (go.samples > 1 || go.shutter > 1)) go.transfer = MARAY_TRANSFER_SRGB;
    maray_report rep{MARAY_REPORT_DURATION_MS, 500};   // Report::Duration(500 ms), examples/maray.rs:77-79
    int rc = 0;
    if (!frames) rc = maray_gen(scene, tex.data(), (uint32_t)tex.size(), &go, rep, output.c_str());
    // FROM + i (TO - FROM) / (FRAMES - 1) in f64; the last frame is TO itself (the range's end, whatever the rounding)
    auto frame_value = [&](uint32_t f) { return frames == 1 ? from : f == frames - 1 ? to : from + (double)f * (to - from) / (double)(frames - 1); };
    if (one_file) {
        // one row of values per image: the animated parameter's, and every other parameter's current value
        uint32_t n_par = 0;
        maray_scene_param_count(scene, &n_par);
        std::vector<double> values((size_t)frames * n_par);
        for (uint32_t f = 0; f < frames; f++)
            for (uint32_t k = 0; k < n_par; k++) {
                double v = 0.0;
                maray_scene_param_info(scene, k, nullptr, nullptr, nullptr, &v);
                values[(size_t)f * n_par + k] = k == anim_index ? frame_value(f) : v;
            }
        ao.container = y4m ? MARAY_CONTAINER_Y4M : MARAY_CONTAINER_APNG;
        rc = maray_gen_animation_ex(scene, tex.data(), (uint32_t)tex.size(), &go, values.data(), frames, fps_den, fps_num, loops, &ao, output.c_str());
    }
    for (uint32_t f = 0; !one_file && f < frames && !rc; f++) {
        const double v = frame_value(f);
        char path[4096];
        snprintf(path, sizeof path, output.c_str(), (int)f);
        rc = maray_scene_set_param(scene, anim_index, v);
        if (!rc) rc = maray_gen(scene, tex.data(), (uint32_t)tex.size(), &go, rep, path);
    }
    if (rc) fprintf(stderr, "Error: %s\n", maray_last_error());
    for (auto p : rasters) maray_free(p);
    maray_scene_free(scene);
    return rc ? 1 : 0;
}
