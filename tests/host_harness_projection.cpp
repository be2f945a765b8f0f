// Test-only: the three host-compilable forms of the projection factor in apex-solver_amd/csrc/ba_device.hpp -- linearize_obs,
// residual_obs, jv_obs -- under every column mask, both camera widths, both template forms (MASKED / not) and both loss
// forms, for tests/test_projection_ref_host.py: the CPU check that the crafted observations of tests/projection_cases.py leave
// the long double reference inside its bound.
#include "ba_device.hpp"
using namespace apex;

namespace {
Cam make_cam(const double* pose, const double* intr, int mask_code) {
    Cam c; load_cam(pose, intr, c);
    c.m_pose = (mask_code & 4) ? 1.0 : 0.0; c.m_lm = (mask_code & 2) ? 1.0 : 0.0; c.m_intr = (mask_code & 1) ? 1.0 : 0.0;
    return c;
}
template <int DC, bool MASKED, class LOSS>
int lin(const Cam& c, const double* pt, const double* uv, LOSS loss, double* r, double* Jc, double* Jl, double* rec4) {
    double jc[2][DC], jl[2][3];
    const bool ok = linearize_obs<DC, MASKED, LOSS>(c, pt, uv[0], uv[1], loss, r, jc, jl, rec4);
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < DC; ++j) Jc[DC * i + j] = jc[i][j];
        for (int j = 0; j < 3; ++j) Jl[3 * i + j] = jl[i][j];
    }
    return ok;
}
template <class LOSS>
int lin_any(int dc, int masked, const Cam& c, const double* pt, const double* uv, LOSS loss, double* r, double* Jc, double* Jl, double* rec4) {
    if (dc == 9) return masked ? lin<9, true, LOSS>(c, pt, uv, loss, r, Jc, Jl, rec4) : lin<9, false, LOSS>(c, pt, uv, loss, r, Jc, Jl, rec4);
    return masked ? lin<6, true, LOSS>(c, pt, uv, loss, r, Jc, Jl, rec4) : lin<6, false, LOSS>(c, pt, uv, loss, r, Jc, Jl, rec4);
}
template <class LOSS>
int jv_any(int dc, int masked, const Cam& c, const double* pt, const double* uv, LOSS loss, const double* a, const double* b, double* u,
           double* w) {
    if (dc == 9)
        return masked ? jv_obs<9, true, LOSS>(c, pt, uv[0], uv[1], loss, a, a + 9, b, b + 9, u, w)
                      : jv_obs<9, false, LOSS>(c, pt, uv[0], uv[1], loss, a, a + 9, b, b + 9, u, w);
    return masked ? jv_obs<6, true, LOSS>(c, pt, uv[0], uv[1], loss, a, a + 6, b, b + 6, u, w)
                  : jv_obs<6, false, LOSS>(c, pt, uv[0], uv[1], loss, a, a + 6, b, b + 6, u, w);
}
}  // namespace

extern "C" {
// kind < 0: the huber_delta form with delta = p0; else the general family.  masked = 0: the MASKED = false instantiation (the
// masks are not read: only meaningful where every block the factor has columns for is optimised).  rec4: the projection record.
// Returns validity, -1 for a refused loss.
int hp_linearize(int dc, int masked, int mask_code, const double* pose, const double* intr, const double* pt, const double* uv, int kind,
                 double p0, double p1, double* r, double* Jc, double* Jl, double* rec4) {
    const Cam c = make_cam(pose, intr, mask_code);
    if (kind < 0) return lin_any<double>(dc, masked, c, pt, uv, p0, r, Jc, Jl, rec4);
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l) || !pg_loss_first_arm_only(l)) return -1;
    return lin_any<const PgLoss&>(dc, masked, c, pt, uv, l, r, Jc, Jl, rec4);
}
int hp_residual(const double* pose, const double* intr, const double* pt, const double* uv, int kind, double p0, double p1, double* r) {
    const Cam c = make_cam(pose, intr, 7);
    if (kind < 0) return residual_obs<double>(c, pt, uv[0], uv[1], p0, r);
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l) || !pg_loss_first_arm_only(l)) return -1;
    return residual_obs<const PgLoss&>(c, pt, uv[0], uv[1], l, r);
}
// u = J a, w = J b for a, b [dc + 3] (camera columns, then the landmark's)
int hp_jv(int dc, int masked, int mask_code, const double* pose, const double* intr, const double* pt, const double* uv, int kind, double p0,
          double p1, const double* a, const double* b, double* u, double* w) {
    const Cam c = make_cam(pose, intr, mask_code);
    if (kind < 0) return jv_any<double>(dc, masked, c, pt, uv, p0, a, b, u, w);
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l) || !pg_loss_first_arm_only(l)) return -1;
    return jv_any<const PgLoss&>(dc, masked, c, pt, uv, l, a, b, u, w);
}
}
