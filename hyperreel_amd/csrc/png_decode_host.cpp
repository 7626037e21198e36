// Host build of hr_png_decode.h for hyperreel_amd/png.py's decode_host and probe-free checks: the same functions the kernels of
// png_decode_kernel.hip call, compiled by the host compiler into a small library of its own.  Pixels and status equal the device's.
#include "hr_png_decode.h"

extern "C" {

// signature and IHDR: the status of hr_png_read_head (0: info is filled)
int32_t hr_png_host_probe(const uint8_t* file, int64_t n, hr_png_info* info) { return hr_png_read_head(file, n, info); }

// out: expect_h * expect_w * out_channels bytes; (-1, -1): the size hr_png_host_probe reports.  Returns the image's status.
int32_t hr_png_host_decode(const uint8_t* file, int64_t n, int32_t expect_w, int32_t expect_h, int32_t out_channels, uint8_t* out, hr_png_info* info)
{
    return hr_png_decode_host_sized(file, n, expect_w, expect_h, out_channels, out, info);
}

}
