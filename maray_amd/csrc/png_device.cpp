// png_device.cpp — the object behind the device PNG encoder (product code; include/maray_hip.h, "device PNG encoder"): it
// owns the kernels' scratch (slots, lengths, offsets, the gathered stream), a band buffer for the entry points that render,
// pinned staging and a stream, cuts a raster into bands of rows, and per band brings first the totals (24 bytes) and then
// exactly the compressed bytes to the host.  png_assemble puts the zlib stream and the container around the pieces.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "png_container.hpp"
#include "png_device.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

void grow(unsigned char *&p, size_t &cap, size_t want)
{
    if (want <= cap) return;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr; cap = 0;
    HIP_TRY(hipMalloc((void **)&p, want));
    cap = want;
}

std::atomic<uint64_t> g_bytes_to_host{0};

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

uint32_t band_rows_from_env()
{
    const char *e = getenv("MARAY_PNG_BAND_ROWS");
    if (!e || atoll(e) <= 0) return 0;
    return (uint32_t)std::min<long long>(atoll(e), 0x7FFFFFFF);
}

// the scratch of a band of `rows` rows: where everything lies, and the kernels' arguments
PngBandArgs band_args(PngEncoder &E, const unsigned char *src, uint32_t w, uint32_t rows)
{
    PngBandArgs a{};
    a.src = src; a.w = w; a.rows = rows;
    a.nseg = png_row_segments(w);
    a.slot_bytes = png_slot_bytes(w);
    const uint64_t n = (uint64_t)rows * a.nseg;
    if (n > 0x7FFFFFFFull) throw Error{MARAY_E_INTERNAL, "device PNG encoder: band too large"};
    a.n_segs = (uint32_t)n;
    const size_t payload = (size_t)n * a.slot_bytes;
    grow(E.slots, E.slots_cap, payload);
    grow(E.stream, E.stream_cap, payload);
    const size_t o_adler = up16((size_t)n * 4), o_off = o_adler + up16((size_t)n * 8), o_tot = o_off + up16((size_t)n * 8);
    grow(E.meta, E.meta_cap, o_tot + 32);
    a.slots = E.slots; a.stream = E.stream;
    a.lens = (uint32_t *)E.meta;
    a.adler = (uint32_t *)(E.meta + o_adler);
    a.offsets = (uint64_t *)(E.meta + o_off);
    a.totals = (uint64_t *)(E.meta + o_tot);
    return a;
}

}   // namespace

PngEncoder::PngEncoder(int dev) : device(dev), band_rows_env(band_rows_from_env())
{
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void **)&h_totals, 32, hipHostMallocDefault));
}

PngEncoder::~PngEncoder()
{
    (void)hipSetDevice(device);
    if (own_stream) { (void)hipStreamSynchronize(own_stream); (void)hipStreamDestroy(own_stream); }
    (void)hipFree(slots); (void)hipFree(stream); (void)hipFree(meta); (void)hipFree(raster);
    if (staging) (void)hipHostFree(staging);
    if (h_totals) (void)hipHostFree(h_totals);
}

// Rows of one band: the byte budget (or MARAY_PNG_BAND_ROWS), and never more than 2^30 filtered bytes, so that every size
// and offset inside a band fits 32 bits with room to spare (past a band they are 64-bit)
uint32_t PngEncoder::band_rows(uint32_t w) const
{
    const uint64_t row = (uint64_t)w * 3 + 1;
    const uint64_t want = band_rows_env ? band_rows_env : std::max<uint64_t>(1, band_bytes / row);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, ((uint64_t)1 << 30) / row));
}

unsigned char *PngEncoder::band_buffer(size_t bytes)
{
    HIP_TRY(hipSetDevice(device));
    grow(raster, raster_cap, bytes);
    return raster;
}

void PngEncoder::encode_rows(const unsigned char *d_rgb8, uint32_t w, uint32_t rows, hipStream_t st, PngPiece &out)
{
    if (!rows || !w) return;
    if (!d_rgb8) throw Error{MARAY_E_ARG, "null argument"};
    HIP_TRY(hipSetDevice(device));
    const uint32_t step = band_rows(w);
    for (uint32_t r0 = 0; r0 < rows; r0 += std::min(step, rows - r0)) {
        const uint32_t n = std::min(step, rows - r0);
        const PngBandArgs a = band_args(*this, d_rgb8 + (size_t)r0 * w * 3, w, n);
        png_band_compress(a, st);
        png_band_scan(a, st);
        png_band_gather(a, st);
        HIP_TRY(hipMemcpyAsync(h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t total = h_totals[0];
        if (total > (uint64_t)a.n_segs * a.slot_bytes) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a band's stream exceeds its bound"};
        if (total > staging_cap) {
            if (staging) HIP_TRY(hipHostFree(staging));
            staging = nullptr; staging_cap = 0;
            const size_t want = std::max<size_t>((size_t)total + (size_t)total / 4, (size_t)1 << 20);
            HIP_TRY(hipHostMalloc((void **)&staging, want, hipHostMallocDefault));
            staging_cap = want;
        }
        HIP_TRY(hipMemcpyAsync(staging, a.stream, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        out.z.insert(out.z.end(), staging, staging + (size_t)total);
        AdlerPart p;
        p.n = (uint32_t)(h_totals[1] & 0xFFFFFFFFu); p.a = (uint32_t)(h_totals[1] >> 32); p.b = (uint32_t)h_totals[2];
        out.adler.append(p);
        g_bytes_to_host += total + 24;
    }
}

void PngEncoder::encode_rendered(uint32_t w, uint32_t y0, uint32_t y1, hipStream_t st,
                                 const std::function<void(uint32_t, uint32_t, unsigned char *, hipStream_t)> &render, PngPiece &out)
{
    if (y0 >= y1 || !w) return;
    HIP_TRY(hipSetDevice(device));
    const uint32_t step = band_rows(w);
    grow(raster, raster_cap, (size_t)std::min(step, y1 - y0) * w * 3);
    for (uint32_t b0 = y0; b0 < y1; b0 += std::min(step, y1 - b0)) {
        const uint32_t b1 = b0 + std::min(step, y1 - b0);
        render(b0, b1, raster, st);
        HIP_TRY(hipSetDevice(device));
        encode_rows(raster, w, b1 - b0, st, out);
    }
}

// ---- the encoders a process keeps ------------------------------------------------------------------------------------
namespace {
std::mutex g_pool_mutex;
// never destroyed: at process exit the HIP runtime may be gone before a static's destructor runs
std::multimap<int, PngEncoder *> &g_pool = *new std::multimap<int, PngEncoder *>();
}   // namespace

PngEncoder *png_encoder_acquire(int device)
{
    const uint32_t env = band_rows_from_env();
    std::vector<PngEncoder *> stale;
    PngEncoder *e = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        for (auto it = g_pool.lower_bound(device); it != g_pool.end() && it->first == device && !e;) {
            if (it->second->band_rows_env == env) e = it->second; else stale.push_back(it->second);
            it = g_pool.erase(it);
        }
    }
    for (PngEncoder *s : stale) delete s;
    return e ? e : new PngEncoder(device);
}

void png_encoder_release(PngEncoder *e)
{
    if (!e) return;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        if (g_pool.count(e->device) < 2) { g_pool.insert({e->device, e}); return; }
    }
    delete e;
}

uint64_t png_bytes_to_host() { return g_bytes_to_host.load(); }
void png_count_bytes_to_host(uint64_t n) { g_bytes_to_host += n; }

void png_check_size(uint32_t w, uint32_t h)
{
    if (w > MARAY_DOMAIN_MAX || h > MARAY_DOMAIN_MAX || ((uint64_t)w * 3 + 1) * h > MARAY_PNG_MAX_BYTES)
        throw Error{MARAY_E_LIMIT, "image too large for the PNG writer"};
}

std::vector<uint8_t> png_close_stream(uint32_t h_end, const std::vector<const PngPiece *> &pieces)
{
    size_t zn = 2 + 5 + 4;
    uint32_t y = pieces.empty() ? 0 : pieces.front()->y0;
    for (const PngPiece *p : pieces) {
        if (p->y0 != y || p->y1 <= p->y0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image in row order"};
        y = p->y1;
        zn += p->z.size();
    }
    if (pieces.empty() || y != h_end) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image"};
    std::vector<uint8_t> z;
    z.reserve(zn);
    z.push_back(0x78); z.push_back(0x01);
    uint32_t s1 = 1, s2 = 0;
    for (const PngPiece *p : pieces) {
        z.insert(z.end(), p->z.begin(), p->z.end());
        s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)p->adler.n * s1 + p->adler.b) % PNG_ADLER_MOD);
        s1 = (s1 + p->adler.a) % PNG_ADLER_MOD;
    }
    static const uint8_t last[5] = {0x01, 0x00, 0x00, 0xFF, 0xFF};       // the final, empty stored block
    z.insert(z.end(), last, last + 5);
    put_be32(z, (s2 << 16) | s1);
    return z;
}

std::vector<uint8_t> png_assemble(uint32_t w, uint32_t h, const std::vector<const PngPiece *> &pieces)
{
    if (!pieces.empty() && pieces.front()->y0 != 0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image in row order"};
    const std::vector<uint8_t> z = png_close_stream(h, pieces);
    return png_file(w, h, z.data(), z.size());
}

float png_time_kernels(int device, const unsigned char *d_rgb8, uint32_t w, uint32_t rows, int reps, uint64_t *stream_bytes)
{
    if (!d_rgb8 || !w || !rows || reps <= 0) throw Error{MARAY_E_ARG, "png_time_kernels: a raster, w, rows and reps > 0"};
    png_check_size(w, rows);
    if (((uint64_t)w * 3 + 1) * rows > ((uint64_t)1 << 30)) throw Error{MARAY_E_LIMIT, "png_time_kernels: more than one band's bytes"};
    PngEncoderLease E(device);
    HIP_TRY(hipSetDevice(device));
    const PngBandArgs a = band_args(*E.e, d_rgb8, w, rows);
    const hipStream_t st = E->own_stream;
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
    auto once = [&] { png_band_compress(a, st); png_band_scan(a, st); png_band_gather(a, st); };
    once();
    HIP_TRY(hipEventRecord(ev.e0, st));
    for (int i = 0; i < reps; i++) once();
    HIP_TRY(hipEventRecord(ev.e1, st));
    HIP_TRY(hipMemcpyAsync(E->h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stream_bytes) *stream_bytes = E->h_totals[0];
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms / (float)reps;
}

}   // namespace maray
