// Test-only: the general-loss forms of residual_obs / linearize_obs (ba_device.hpp) and pg_loss_first_arm_only (pg_loss.hpp)
// compiled for the HOST, so that the per-lane math of the general BA kernels can be compared with tests/np_ref_ba_loss.py
// without a GPU.
#include "ba_device.hpp"
using namespace apex;
extern "C" {
// -1: pg_loss_make refuses; else pg_loss_first_arm_only
int hb_first_arm_only(int kind, double p0, double p1) {
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return -1;
    return pg_loss_first_arm_only(l) ? 1 : 0;
}
// r[2], Jc[2][dc], Jl[2][3], rec4[4] of one observation under the loss; pose7 raw, as load_cam takes it
int hb_linearize_obs(int dc, const double* pose, const double* intr, const double* pt, const double* uv, int kind, double p0,
                     double p1, double* r, double* Jc, double* Jl, double* rec4) {
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return -1;
    Cam c; load_cam(pose, intr, c);
    double jl[2][3]; bool ok;
    if (dc == 9) { double jc[2][9]; ok = linearize_obs<9>(c, pt, uv[0], uv[1], l, r, jc, jl, rec4);
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 9; ++j) Jc[9 * i + j] = jc[i][j]; }
    else { double jc[2][6]; ok = linearize_obs<6>(c, pt, uv[0], uv[1], l, r, jc, jl, rec4);
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 6; ++j) Jc[6 * i + j] = jc[i][j]; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) Jl[3 * i + j] = jl[i][j];
    return ok;
}
int hb_residual_obs(const double* pose, const double* intr, const double* pt, const double* uv, int kind, double p0, double p1,
                    double* r) {
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return -1;
    Cam c; load_cam(pose, intr, c);
    return residual_obs(c, pt, uv[0], uv[1], l, r);
}
}
