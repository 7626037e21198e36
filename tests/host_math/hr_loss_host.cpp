// TEST-ONLY host build of hyperreel_amd/csrc/hr_loss.h (the loss arithmetic the loss kernel calls), so that the CPU suite can compare it
// with the reference's fixtures without a GPU.  Nothing in the product links or loads this file.
#include <stddef.h>

#include "../../hyperreel_amd/csrc/hr_loss.h"

extern "C" {

int hl_sizeof_out() { return (int)sizeof(hr_loss_out); }
int hl_offsetof_out(int i)
{
    switch (i) {
        case 0: return (int)offsetof(hr_loss_out, loss_sum);
        case 1: return (int)offsetof(hr_loss_out, sse);
        case 2: return (int)offsetof(hr_loss_out, loss);
        case 3: return (int)offsetof(hr_loss_out, pad);
        default: return -1;
    }
}
int hl_abi_version() { return HR_ABI_VERSION; }
int hl_type_code(int i)
{
    const int codes[6] = {HR_LOSS_MSE, HR_LOSS_WEIGHTED_MSE, HR_LOSS_MAE, HR_LOSS_WEIGHTED_MAE, HR_LOSS_HUBER, HR_LOSS_PREMULTIPLIED};
    return i >= 0 && i < 6 ? codes[i] : -1;
}
int hl_type_valid(int32_t type) { return hr_loss_type_valid(type); }
int64_t hl_blocks(int64_t n_rays) { return hr_loss_blocks(n_rays); }

// hr_image_loss on the host: the elements in index order, the sums in double.  weight, upstream and d_pred may be NULL as in the C ABI.
void hl_image_loss(const float* pred, const float* gt, const float* weight, int64_t n_rays, int32_t type, float delta, const float* upstream,
                   hr_loss_out* out, float* d_pred)
{
    const float s = hr_loss_mean_scale(n_rays), up = upstream ? upstream[0] : 1.0f;
    double loss_sum = 0.0, sse = 0.0;
    for (int64_t i = 0; i < 3 * n_rays; ++i) {
        float term, sq, grad;
        hr_loss_element(type, delta, s, pred[i], gt[i], weight ? weight[i / 3] : 1.0f, &term, &sq, &grad);
        loss_sum += (double)term;
        sse += (double)sq;
        if (d_pred) d_pred[i] = grad * up;
    }
    hr_loss_result(loss_sum, sse, n_rays, out);
}

}
