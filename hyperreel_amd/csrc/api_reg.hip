// C ABI, the TensoRF regulariser of a training step: hr_reg_plan_create / hr_tensorf_reg / hr_reg_plan_destroy (kernels: reg_kernel.hip).
// The plan holds what the host decides -- the checked descriptor table, the workgroup prefix table, which tensors take the 16-byte
// path -- and the workspace of per-workgroup partial sums, so that the call itself only enqueues two kernels on `stream`.
#include <hip/hip_runtime.h>

#include <memory>

#include "hr_model.h"

struct hr_reg_plan {
    HrRegBatch batch = {};
    DevMem<float> partials;                 // 3 floats per workgroup
};

// the checked table -> the launch's batch; nothing is allocated
static int fill_batch(const char* who, const hr_reg_tensor* tensors, int32_t n_tensors, HrRegBatch& b)
{
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return fail(HR_E_INVALID, "%s: null argument (tensors)", who);
    if (n_tensors > HR_REG_MAX_TENSORS) return fail(HR_E_INVALID, "%s: %d tensors, at most %d in one call", who, (int)n_tensors, HR_REG_MAX_TENSORS);
    b = HrRegBatch();
    b.count = 0;
    b.first_block[0] = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const hr_reg_tensor& t = tensors[i];
        if (t.channels < 0) return fail(HR_E_INVALID, "%s: tensor %d has %d channels", who, i, (int)t.channels);
        if (t.h < 1 || t.w < 1) return fail(HR_E_INVALID, "%s: tensor %d is %d x %d (h, w): at least 1 x 1", who, i, (int)t.h, (int)t.w);
        for (int32_t s : {t.slot_h, t.slot_w, t.slot_l})
            if (s < -1 || s >= HR_REG_SLOTS) return fail(HR_E_INVALID, "%s: tensor %d reads weight slot %d of %d", who, i, (int)s, HR_REG_SLOTS);
        if ((t.slot_h >= 0 || t.slot_w >= 0) && (t.h < 2 || t.w < 2))
            return fail(HR_E_INVALID, "%s: tensor %d has a total-variation term and is %d x %d (h, w): the reference divides by a zero count below 2 x 2",
                        who, i, (int)t.h, (int)t.w);
        if (t.channels == 0) continue;              // the reference's n_comp == 0 planes: skipped
        if (!t.plane_dev) return fail(HR_E_INVALID, "%s: tensor %d has a null plane", who, i);
        if (!t.grad_dev) return fail(HR_E_INVALID, "%s: tensor %d has a null gradient", who, i);
        const int64_t n = (int64_t)t.channels * t.h * t.w;
        const int64_t blocks = (n + HR_REG_BLOCK - 1) / HR_REG_BLOCK;
        if ((int64_t)b.first_block[b.count] + blocks > 0x3fffffff) return fail(HR_E_INVALID, "%s: tensor %d is too large for one launch", who, i);
        const int k = b.count++;
        b.p[k] = t.plane_dev; b.g[k] = t.grad_dev; b.n[k] = n; b.H[k] = t.h; b.W[k] = t.w;
        b.kh[k] = t.kh; b.kw[k] = t.kw; b.kl[k] = t.kl;
        b.sh[k] = t.slot_h; b.sw[k] = t.slot_w; b.sl[k] = t.slot_l;
        b.vec4[k] = (t.w % 4 == 0) && (reinterpret_cast<uintptr_t>(t.plane_dev) % 16 == 0) && (reinterpret_cast<uintptr_t>(t.grad_dev) % 16 == 0);
        b.first_block[k + 1] = b.first_block[k] + (int)blocks;
    }
    return HR_OK;
}

int hr_reg_plan_create(const hr_reg_tensor* tensors, int32_t n_tensors, hr_reg_plan** out)
{
    if (!out) return fail(HR_E_INVALID, "hr_reg_plan_create: null argument (out)");
    *out = nullptr;
    std::unique_ptr<hr_reg_plan> plan(new hr_reg_plan());
    if (int rc = fill_batch("hr_reg_plan_create", tensors, n_tensors, plan->batch)) return rc;
    const size_t blocks = (size_t)plan->batch.first_block[plan->batch.count];
    if (blocks > 0) {
        const hipError_t e = plan->partials.alloc(sizeof(float) * 3 * blocks);
        if (e != hipSuccess) return fail(HR_E_HIP, "hr_reg_plan_create: %s", hipGetErrorString(e));
    }
    *out = plan.release();
    return HR_OK;
}

int hr_reg_plan_update(hr_reg_plan* plan, const hr_reg_tensor* tensors, int32_t n_tensors)
{
    if (!plan) return fail(HR_E_INVALID, "hr_reg_plan_update: null argument (plan)");
    HrRegBatch b;
    if (int rc = fill_batch("hr_reg_plan_update", tensors, n_tensors, b)) return rc;
    const HrRegBatch& old = plan->batch;
    bool same = b.count == old.count;
    for (int k = 0; same && k < b.count; ++k) same = b.n[k] == old.n[k] && b.H[k] == old.H[k] && b.W[k] == old.W[k];
    if (!same) return fail(HR_E_INVALID, "hr_reg_plan_update: the tensors' shapes differ from the plan's: create a new plan");
    plan->batch = b;
    return HR_OK;
}

int hr_tensorf_reg(const hr_reg_plan* plan, const float* weights_dev, float* loss_dev, int32_t add_grad, void* stream)
{
    if (!plan) return fail(HR_E_INVALID, "hr_tensorf_reg: null argument (plan)");
    if (!weights_dev) return fail(HR_E_INVALID, "hr_tensorf_reg: null argument (weights_dev)");
    if (!loss_dev) return fail(HR_E_INVALID, "hr_tensorf_reg: null argument (loss_dev)");
    hr_launch_tensorf_reg(plan->batch, weights_dev, plan->partials, loss_dev, add_grad ? 1 : 0, (hipStream_t)stream);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

void hr_reg_plan_destroy(hr_reg_plan* plan) { delete plan; }
