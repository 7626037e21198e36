// TEST-ONLY host build of hyperreel_amd/csrc/hr_plan.h (plane-pair geometry, plane class, the training step's launch plan), so that
// the suites ask the library's own code which branch a case takes.  Nothing in the product links or loads this file.
#include "../../hyperreel_amd/csrc/hr_plan.h"

extern "C" {

int hp_sizeof_plane() { return (int)sizeof(HrGridPlane); }
int hp_sizeof_plan() { return (int)sizeof(HrTrainPlan); }
int hp_round_zp(int z_channels) { return hr_round_zp(z_channels); }

int hp_plane_geometry(const hr_config* c, HrGridPlane* out, int* ca_total, int* n_basis_cols)
{
    return hr_plane_geometry(*c, out, ca_total, n_basis_cols) ? 1 : 0;
}

// train: the size predicate of the training step's class path instead of the render gathers'
int hp_plane_class(const HrGridPlane* planes, int ca_total, int train)
{
    return train ? hr_plane_class(planes, ca_total, hr_plane_fits_train) : hr_plane_class(planes, ca_total, hr_plane_fits_gather);
}

// The plan of hr_train_backward for n_rays rays of a finalized model of *c: a backward step whose tape has taps, point gradient
// and grouped order (the workspace provides them), float or 64-bit fixed-point accumulators.  256 compute units: no branch depends
// on the count, only grid sizes do.
void hp_train_plan(const hr_config* c, long long n_rays, int deterministic, HrTrainPlan* out)
{
    HrGridPlane planes[3];
    int ca_total = 0, n_basis_cols = 0;
    (void)hr_plane_geometry(*c, planes, &ca_total, &n_basis_cols);
    const HrTrainPlanIn in = {n_rays, true, true, true, true, deterministic != 0, deterministic ? sizeof(long long) : sizeof(float), 256};
    *out = hr_train_plan(*c, planes, ca_total, n_basis_cols, in);
}

}  // extern "C"
