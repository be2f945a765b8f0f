/* The camera-prior calls of the C ABI from plain C (tests/test_gpu_ba_priors.py compiles and runs this against include/apexgpu.h
 * and libapexgpu.so).  Input: one binary file -- int64 {n_cam, n_pt, n_obs, n_pose, n_intr}, cam_idx, pt_idx (uint32), obs_uv,
 * poses [n_cam][7], intr [n_cam][3], points [n_pt][3], then per prior set: cam (uint32), data, huber delta, weight.
 * Output: one JSON line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "apexgpu.h"

static void* take(FILE* f, size_t n, size_t size) {
    void* p = malloc((n && size) ? n * size : 1);
    if (!p || fread(p, size, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return p;
}

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ != APEXGPU_OK) { fprintf(stderr, "%s: %d %s\n", #call, rc_, apexgpu_last_error(h)); return 1; } \
    } while (0)

static double norm(const double* x, int64_t n) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i] * x[i];
    return sqrt(s);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t* hd = take(f, 5, sizeof(int64_t));
    const int64_t n_cam = hd[0], n_pt = hd[1], n_obs = hd[2], n_pose = hd[3], n_intr = hd[4];
    uint32_t* cam_idx = take(f, n_obs, 4); uint32_t* pt_idx = take(f, n_obs, 4);
    double* uv = take(f, 2 * n_obs, 8); double* poses = take(f, 7 * n_cam, 8); double* intr = take(f, 3 * n_cam, 8); double* pts = take(f, 3 * n_pt, 8);
    uint32_t* pc = take(f, n_pose, 4); double* pd = take(f, 7 * n_pose, 8); double* pdl = take(f, n_pose, 8); double* pw = take(f, n_pose, 8);
    uint32_t* ic = take(f, n_intr, 4); double* id = take(f, 3 * n_intr, 8); double* idl = take(f, n_intr, 8); double* iw = take(f, n_intr, 8);
    fclose(f);

    apexgpu_solver* h = NULL;
    if (apexgpu_create(n_cam, n_pt, n_obs, APEXGPU_MODE_SELF_CALIBRATION, 0, &h) != APEXGPU_OK) return 1;
    int64_t* intr_col = malloc(n_cam * 8); int64_t* pose_col = malloc(n_cam * 8); int64_t* pt_col = malloc(n_pt * 8);
    CHECK(apexgpu_reference_columns(n_cam, n_pt, intr_col, pose_col, pt_col));
    CHECK(apexgpu_set_structure(h, cam_idx, pt_idx, uv, intr_col, pose_col, pt_col, NULL, NULL, NULL, -1.0));
    CHECK(apexgpu_set_params(h, poses, intr, pts));
    const uint32_t bad = (uint32_t)n_cam;
    const int bad_rc = apexgpu_set_pose_priors(h, 1, &bad, pd, NULL, NULL);
    CHECK(apexgpu_set_pose_priors(h, n_pose, pc, pd, pdl, pw));
    CHECK(apexgpu_set_intrinsic_priors(h, n_intr, ic, id, idl, iw));
    double cost = 0.0, cleared = 0.0;
    CHECK(apexgpu_cost(h, &cost));
    double* rp = malloc((7 * n_pose + 1) * 8); double* ri = malloc((3 * n_intr + 1) * 8);
    CHECK(apexgpu_get_prior_residual(h, rp, ri));
    const int64_t n = 9 * n_cam + 3 * n_pt;
    double* step = malloc(n * 8);
    CHECK(apexgpu_solve_augmented(h, 1e4, APEXGPU_VARIANT_SPARSE, step, NULL));
    CHECK(apexgpu_set_pose_priors(h, 0, NULL, NULL, NULL, NULL));
    CHECK(apexgpu_set_intrinsic_priors(h, 0, NULL, NULL, NULL, NULL));
    CHECK(apexgpu_cost(h, &cleared));
    printf("{\"cost\": %.17g, \"cleared_cost\": %.17g, \"step_norm\": %.17g, \"pose_r_norm\": %.17g, \"intr_r_norm\": %.17g, \"bad_camera\": %d}\n",
           cost, cleared, norm(step, n), norm(rp, 7 * n_pose), norm(ri, 3 * n_intr), bad_rc);
    apexgpu_destroy(h);
    return 0;
}
