// Test-only: jv_obs against linearize_obs (ba_device.hpp), both compiled for the HOST.  jv_obs forms the entries of the corrected
// Jacobian a second time and accumulates them; this harness ties the two together: with unit vectors for a and b, jv_obs must
// hand back every entry of linearize_obs' Jc and Jl with the same bits.
#include "ba_device.hpp"
using namespace apex;

template <int DC, class LOSS>
static int compare(const Cam& c, const double* pt, const double* uv, LOSS loss, double* J_lin, double* J_jv) {
    double r[2], jc[2][DC], jl[2][3];
    const bool ok = linearize_obs<DC>(c, pt, uv[0], uv[1], loss, r, jc, jl);
    constexpr int N = DC + 3;
    for (int rr = 0; rr < 2; ++rr) {
        for (int k = 0; k < DC; ++k) J_lin[N * rr + k] = jc[rr][k];
        for (int k = 0; k < 3; ++k) J_lin[N * rr + DC + k] = jl[rr][k];
    }
    int bad = 0;
    for (int k = 0; k < N; ++k) {   // a = e_k, b = e_(N-1-k): both outputs are checked
        double a[N] = {}, b[N] = {}, u[2], w[2];
        a[k] = 1.0; b[N - 1 - k] = 1.0;
        const bool ok2 = jv_obs<DC>(c, pt, uv[0], uv[1], loss, a, a + DC, b, b + DC, u, w);
        if (ok2 != ok) ++bad;
        for (int rr = 0; rr < 2; ++rr) {
            J_jv[N * rr + k] = u[rr];
            if (!(u[rr] == J_lin[N * rr + k])) ++bad;
            if (!(w[rr] == J_lin[N * rr + N - 1 - k])) ++bad;
        }
    }
    return ok ? bad : bad + 1000;   // (+1000: the projection is invalid, every entry must be zero)
}

extern "C" {
// kind < 0: the huber_delta form with delta = p0; else the general form.  mask_code = 4 POSE + 2 LANDMARK + INTRINSIC.
// J_lin / J_jv [2][dc + 3]: camera columns, then the landmark's.  Returns the number of entries that differ (+1000 when invalid).
int hj_compare(int dc, int mask_code, const double* pose, const double* intr, const double* pt, const double* uv, int kind, double p0,
               double p1, double* J_lin, double* J_jv) {
    Cam c; load_cam(pose, intr, c);
    c.m_pose = (mask_code & 4) ? 1.0 : 0.0; c.m_lm = (mask_code & 2) ? 1.0 : 0.0; c.m_intr = (mask_code & 1) ? 1.0 : 0.0;
    if (kind < 0) return dc == 9 ? compare<9>(c, pt, uv, p0, J_lin, J_jv) : compare<6>(c, pt, uv, p0, J_lin, J_jv);
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return -1;
    return dc == 9 ? compare<9, const PgLoss&>(c, pt, uv, l, J_lin, J_jv) : compare<6, const PgLoss&>(c, pt, uv, l, J_lin, J_jv);
}
// u[2], w[2] of jv_obs for general a, b [dc + 3] (huber_delta form)
int hj_jv(int dc, const double* pose, const double* intr, const double* pt, const double* uv, double delta, const double* a,
          const double* b, double* u, double* w) {
    Cam c; load_cam(pose, intr, c);
    return dc == 9 ? jv_obs<9>(c, pt, uv[0], uv[1], delta, a, a + 9, b, b + 9, u, w) : jv_obs<6>(c, pt, uv[0], uv[1], delta, a, a + 6, b, b + 6, u, w);
}
}
