// Host build of hr_jpeg_encode.h for hyperreel_amd/jpeg.py's encode_host: the same functions the kernels of jpeg_encode_kernel.hip call,
// compiled by the host compiler into a small library of its own (libhyperreel_hip.so holds device code only).  The file's bytes equal
// the device's.
#include "hr_jpeg_encode.h"

extern "C" {

// -1 for arguments the encoders refuse
int64_t hr_jpeg_host_bound(int32_t w, int32_t h, int32_t channels, int32_t subsampling, int32_t restart_rows)
{
    return hr_jpeg_enc_refusal(w, h, channels, 90, subsampling, restart_rows) ? -1 : hr_jpeg_enc_plan(w, h, channels, subsampling, restart_rows).bound;
}

// pixel_type as hr_jpeg_encode's; returns the file's length, or -1 for refused arguments or a capacity below the bound.  stats (may be
// NULL): int64 stuffed bytes, F0 codes, then int32 largest DC and AC category
int64_t hr_jpeg_host_encode(const void* pixels, int32_t pixel_type, int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling,
                            int32_t restart_rows, uint8_t* file, int64_t capacity, hr_jpeg_enc_stats* stats)
{
    return hr_jpeg_encode_host(pixels, pixel_type, w, h, channels, quality, subsampling, restart_rows, file, capacity, nullptr, stats);
}

}
