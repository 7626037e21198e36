// Host build of hr_png.h for hyperreel_amd/png.py's encode_host: the same functions the kernels of png_kernel.hip call, compiled by the
// host compiler into a small library of its own (libhyperreel_hip.so holds device code only).  The file's bytes equal the device's.
#include "hr_png.h"

extern "C" {

// -1 for a shape the encoders refuse
int64_t hr_png_host_bound(int32_t w, int32_t h, int32_t channels) { return hr_png_shape_ok(w, h, channels) ? hr_png_plan(w, h, channels).bound : -1; }

// pixel_type, filter_mode as hr_png_encode's; returns the file's length, or -1 for a refused shape or a capacity below the bound.  The
// three outputs may be NULL: the filtered bytes (h * (1 + w c)), the tokens (as many uint16), the rows' filter types (h).
int64_t hr_png_host_encode(const void* pixels, int32_t pixel_type, int32_t filter_mode, int32_t w, int32_t h, int32_t channels, uint8_t* file,
                           int64_t capacity, uint8_t* filtered_out, uint16_t* tokens_out, uint8_t* row_filters_out)
{
    return hr_png_encode_host(pixels, pixel_type, filter_mode, w, h, channels, file, capacity, filtered_out, tokens_out, row_filters_out);
}

}
