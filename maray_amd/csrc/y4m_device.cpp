// y4m_device.cpp — the object behind the raw-video entry points (product code; include/maray_hip.h, "raw video"): two
// buffers of Y'CbCr planes in HBM and two in pinned host memory.  Frame k is converted into buffer k & 1 on the caller's
// stream (yuv.hip); an event lets the copy stream bring the planes to the host; then the calling thread waits for frame
// k - 1's copy -- enqueued a frame earlier -- and hands `FRAME\n` and its planes to the sink while frame k's kernels run.
// A buffer is reused two frames later, after its frame was handed over: the host's wait orders that.
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "y4m_device.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

}   // namespace

hipStream_t y4m_render_stream(int device)
{
    static std::mutex m;
    static std::map<int, hipStream_t> &streams = *new std::map<int, hipStream_t>();
    std::lock_guard<std::mutex> lk(m);
    auto it = streams.find(device);
    if (it != streams.end()) return it->second;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreate(&st));
    streams[device] = st;
    return st;
}

void y4m_check_timing(uint32_t n_frames, uint32_t delay_num, uint32_t delay_den)
{
    if (!n_frames) throw Error{MARAY_E_ARG, "an animation needs at least one image"};
    if (delay_num > 65535 || delay_den > 65535) throw Error{MARAY_E_ARG, "delay_num and delay_den must fit 16 bits"};
    if (!delay_num) throw Error{MARAY_E_ARG, "a Y4M frame rate is delay_den / delay_num: delay_num must not be 0"};
}

std::string y4m_header(uint32_t w, uint32_t h, uint32_t delay_num, uint32_t delay_den, uint32_t sampling)
{
    // (Y4M has no tag for the matrix: the caller tells the consumer which one it chose)
    return "YUV4MPEG2 W" + std::to_string(w) + " H" + std::to_string(h) + " F" + std::to_string(delay_den ? delay_den : 100u) + ":" +
           std::to_string(delay_num) + " Ip A1:1 " + (sampling == MARAY_YCC_444 ? "C444" : "C420jpeg") + " XCOLORRANGE=LIMITED\n";
}

Y4mWriter::Y4mWriter(int device_, uint32_t w_, uint32_t h_, uint32_t n_frames_, uint32_t delay_num, uint32_t delay_den, uint32_t sampling_,
                     uint32_t matrix_, Sink sink_)
    : device(device_), w(w_), h(h_), n_frames(n_frames_), sampling(sampling_), matrix(matrix_), frame_bytes(ycc_frame_bytes(w_, h_, sampling_)),
      sink(std::move(sink_))
{
    if (sampling != MARAY_YCC_420 && sampling != MARAY_YCC_444) throw Error{MARAY_E_ARG, "unknown Y'CbCr sampling"};
    if (matrix != MARAY_YCC_BT601 && matrix != MARAY_YCC_BT709) throw Error{MARAY_E_ARG, "unknown Y'CbCr matrix"};
    y4m_check_timing(n_frames, delay_num, delay_den);
    ycc_check_frame(w, h);
    header = y4m_header(w, h, delay_num, delay_den, sampling);
    HIP_TRY(hipSetDevice(device));
    try {
        HIP_TRY(hipStreamCreateWithFlags(&copy_st, hipStreamNonBlocking));
        for (uint32_t k = 0; k < (n_frames > 1 ? 2u : 1u); k++) {
            HIP_TRY(hipMalloc((void **)&d_planes[k], frame_bytes));
            HIP_TRY(hipHostMalloc((void **)&h_planes[k], frame_bytes, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&converted[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        }
    } catch (...) {
        release();
        throw;
    }
}

Y4mWriter::~Y4mWriter() { release(); }

void Y4mWriter::release()
{
    (void)hipSetDevice(device);
    if (copy_st) { (void)hipStreamSynchronize(copy_st); (void)hipStreamDestroy(copy_st); }
    (void)hipFree(d_rgb);
    for (int k = 0; k < 2; k++) {
        (void)hipFree(d_planes[k]);
        if (h_planes[k]) (void)hipHostFree(h_planes[k]);
        if (converted[k]) (void)hipEventDestroy(converted[k]);
        if (copied[k]) (void)hipEventDestroy(copied[k]);
        d_planes[k] = h_planes[k] = nullptr; converted[k] = copied[k] = nullptr;
    }
    d_rgb = nullptr; copy_st = nullptr;
}

unsigned char *Y4mWriter::raster()
{
    if (!d_rgb) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc((void **)&d_rgb, (size_t)w * 3 * h));
    }
    return d_rgb;
}

void Y4mWriter::write_one()
{
    const uint32_t k = written & 1u;
    HIP_TRY(hipEventSynchronize(copied[k]));
    if (!written) sink(header.data(), header.size());
    sink("FRAME\n", 6);
    sink(h_planes[k], frame_bytes);
    written++;
}

void Y4mWriter::add_frame(const unsigned char *d_rgb8, hipStream_t st)
{
    if (added >= n_frames) throw Error{MARAY_E_INTERNAL, "raw-video writer: more frames than announced"};
    HIP_TRY(hipSetDevice(device));
    const uint32_t k = added & 1u;
    rgb_to_ycc(d_rgb8, w, h, sampling, matrix, d_planes[k], st);
    HIP_TRY(hipEventRecord(converted[k], st));
    HIP_TRY(hipStreamWaitEvent(copy_st, converted[k], 0));
    HIP_TRY(hipMemcpyAsync(h_planes[k], d_planes[k], frame_bytes, hipMemcpyDeviceToHost, copy_st));
    HIP_TRY(hipEventRecord(copied[k], copy_st));
    added++;
    if (added > 1) write_one();         // the frame before this one, while this one's kernels and copy run
}

void Y4mWriter::finish()
{
    if (added != n_frames) throw Error{MARAY_E_INTERNAL, "raw-video writer: fewer frames than announced"};
    while (written < added) write_one();
}

}   // namespace maray
