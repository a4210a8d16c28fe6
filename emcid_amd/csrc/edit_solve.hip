// Stage 2 of EMCID on gfx950, one edited layer at a time: the primal solver (assemble A = lam*C' + K K^T, factor, solve with the
// N concept columns as right-hand sides, dW = R X^T and the in-place fp32 weight update), the covariance-factor workspace the
// dual forms share (factor, explicit inverse, rescale), and the three dual (Woodbury) forms: adj_k, apply-only, column-sharded.
// Replaces emcid/emcid_main.py:1016-1061 of the reference (torch.linalg.solve + `@` in fp64).  The dense algebra underneath is
// spd_solve.hip's; edit sessions build on the apply-only form in session.hip.
#include "spd_solve.h"

namespace emcid {

// ---- element-wise preparation ---------------------------------------------------------------------

// Kt64[n][j] = double(K[n][j]) * s * g (zero padded to [Np][dp]);
// Rt[n][i]   = double(zs_t[n][i] - Zc[n][i]) * s / layers_left * g  (fp32 subtract first, like the reference).
// g = 1 for the direct solver.  The dual solver passes g = sqrt(lam_factored / lam): it then works with a factor of
// lam_factored * C' whatever the call's lam is (chol(lam C') = sqrt(lam) chol(C')), see emcid_factor_cov_f64.
__global__ __launch_bounds__(256) void prep_kr_kernel(const float* __restrict__ K, const float* __restrict__ Zc,
                                                       const float* __restrict__ zs_t, int N, int d, int h, double s,
                                                       double layers_left, double* __restrict__ Kt64, int Np, int dp,
                                                       double* __restrict__ Rt, int hp, double g = 1.0) {
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < dp; j += 256) {
        double v = 0.0;
        if (n < N && j < d) v = (double)K[(int64_t)n * d + j] * s * g;
        Kt64[(int64_t)n * dp + j] = v;
    }
    if (Rt) {
        for (int i = threadIdx.x; i < hp; i += 256) {
            double v = 0.0;
            if (n < N && i < h) {
                const float src = zs_t[(int64_t)n * h + i] - Zc[(int64_t)n * h + i];
                v = ((double)src * s) / layers_left * g;
            }
            Rt[(int64_t)n * hp + i] = v;
        }
    }
}

// the one launch of prep_kr_kernel: s = sqrt(edit_weight / 0.5) as the reference scales keys and residuals, `gain` the kernel's g
static void launch_prep_kr(const float* K, const float* Zc, const float* zs_t, int64_t N, int64_t d, int64_t h, double edit_weight,
                           int layers_left, double gain, double* Kt, int64_t Np, int64_t dp, double* R, int64_t hp, hipStream_t st) {
    ScopedProf sp(KC_PREP, st);
    hipLaunchKernelGGL(prep_kr_kernel, dim3((unsigned)Np), dim3(256), 0, st, K, Zc, zs_t, (int)N, (int)d, (int)h, sqrt(edit_weight / 0.5),
                       (double)layers_left, Kt, (int)Np, (int)dp, R, (int)hp, gain);
}

__global__ __launch_bounds__(256) void axpy_f32_kernel(float* __restrict__ W, const float* __restrict__ dW, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) W[i] += dW[i];
}

// W = W0 + float(U) ; dW = float(U)   (after the partial U of the concept shards were summed)
__global__ __launch_bounds__(256) void apply_u_kernel(const double* __restrict__ U, const float* __restrict__ W0,
                                                       float* __restrict__ W, float* __restrict__ dW, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const float f = (float)U[i];
        if (dW) dW[i] = f;
        if (W) W[i] = W0[i] + f;
    }
}

// factor + solve of the primal form as one cached hipGraph
static int factor_and_solve(double* A, double* L, int64_t dp, int64_t lda, double* invw, int* info, double* B, double* Y,
                            int64_t rows, int64_t ldb, hipStream_t st) {
    return with_graph(make_key(GRAPH_FACTOR_SOLVE, {A, L, invw, info, B, Y}, {dp, lda, rows, ldb}), st, [&](hipStream_t s) {
        EMCID_TRY(cholesky_impl(A, L, dp, lda, invw, info, s));
        return cholesky_solve_impl(L, dp, lda, invw, B, Y, rows, ldb, s);
    });
}

// ---- dual (Woodbury) solver -----------------------------------------------------------------------------------------
// A = M + Kt^T Kt with M = lam*C' independent of the concepts.  Then  Xt = Kt A^-1 = (I + Pt Kt^T)^-1 Pt,  Pt = Kt M^-1:
// the d x d factorization is of M only — done for ALL edited layers at once, batched, before (and concurrently with)
// the forward pass — and each layer factors just the Np x Np matrix S = I + Pt Kt^T.

// M[l] = lam * double(fl32(fl32(C[l]*cw)/0.5f)) on the lower triangle, identity on the padding (as EpiAssemble)
struct CovPtrs { const float* c[32]; };
__global__ __launch_bounds__(256) void scale_cov_kernel(CovPtrs cov, int d, int dp, double lam, float cw, double* __restrict__ M,
                                                         int64_t s_mat) {
    const int l = blockIdx.y;
    const int i = blockIdx.x;
    const float* C = cov.c[l];
    double* row = M + l * s_mat + (int64_t)i * dp;
    for (int j = threadIdx.x; j <= i; j += 256) {
        double v;
        if (i < d) {
            const float c1 = C[(int64_t)i * d + j] * cw;
            v = lam * (double)(c1 / 0.5f);
        } else {
            v = (i == j) ? 1.0 : 0.0;
        }
        row[j] = v;
    }
}

// S[Np, Np] = I + P Q^T on the lower tiles, K = dp deep.  Np x Np is too few output tiles for the chip, so the
// contraction is split over workgroups that add their partials into the identity with f64 atomics.
static void assemble_dual_system(const double* P, const double* Q, int64_t dp, double* S, int Np, hipStream_t st,
                                 double* sk_work = nullptr) {
    ScopedProf sp(KC_ASSEMBLE, st);
    GemmShape g{P, dp, Q, dp, Np, Np, (int)dp, 1};
    // S = I + P Q^T written once per tile, no identity pass (unless there are more tiles than ticket counters)
    if (Np >= 512 && sk_work && launch_gemm_f64_streamk2<true, true>(g, EpiAxpby{S, Np, 1.0, 0.0}, st, kStreamKWgs, sk_work, 1.0))
        return;
    hipLaunchKernelGGL(eye_f64_kernel, dim3((unsigned)Np), dim3(256), 0, st, S, Np);
    const int kt = (int)(dp / 16);
    g.ksplit = kt >= 64 ? 4 : kt >= 32 ? 2 : 1;
    launch_gemm_f64<true, true>(g, EpiAxpby{S, Np, 1.0, 1.0}, st, Np >= 512 ? 1 : 2);
}

__global__ __launch_bounds__(256) void transpose_f64_kernel(const double* __restrict__ src, int64_t lds_, double* __restrict__ dst,
                                                             int64_t ldd, int rows, int cols) {
    __shared__ double tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (by + r < rows && bx + tx < cols) ? src[(int64_t)(by + r) * lds_ + bx + tx] : 0.0;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (bx + r < cols && by + tx < rows) dst[(int64_t)(bx + r) * ldd + by + tx] = tile[tx][r];
}

struct EditWorkspace {
    int64_t Np, dp, hp;
    int64_t off_A, off_L, off_inv, off_B, off_Y, off_R, total;  // in doubles
    EditWorkspace(int64_t N, int64_t d, int64_t h) {
        Np = round_up(N, NPAD);
        dp = round_up(d, NB);
        hp = round_up(h, 2);
        int64_t o = 0;
        off_A = o; o += dp * dp;
        off_L = o; o += dp * dp;
        off_inv = o; o += inv_doubles(dp);
        off_B = o; o += Np * dp;
        off_Y = o; o += Np * dp;
        off_R = o; o += Np * hp;
        total = o;
    }
};

// RT[h, Np] = Rt^T, then RT := Z^T = RT S^-1 for S = LS LS^T (Y2 [h, Np] is scratch).  As block substitution the solve is 6
// dependent launches on h rows (~140 us at N = 1000, latency-bound); against an explicit XS = inv(LS) it is two GEMMs against a
// triangle, Z^T = (RT XS^T) XS.  XT: XS transposed, as it rode in the factorization (XrowJob), or nullptr when the fused schedule
// did not run.  Then XS is built into `full_inv` [Np, Np] (the callers pass S, which the factorization has consumed) up to
// Np = 4096 and where the y2_doubles of Y2 hold that build's scratch; beyond that, or without `full_inv`, the substitution stays
// (schur_rhs_form, spd_solve.h).
int solve_schur_rhs(const double* R, int64_t hp, int64_t h, int64_t Np, const double* LS, const double* invS, const double* XT,
                    double* full_inv, double* RT, double* Y2, int64_t y2_doubles, hipStream_t st) {
    if (y2_doubles < hp * Np) return fail(EMCID_ERR_WORKSPACE, __func__, "RT / Y2 hold fewer than h rows of Np (h > d rounded up to 128)");
    const int form = schur_rhs_form(Np, XT != nullptr, full_inv != nullptr, y2_doubles);
    hipLaunchKernelGGL(transpose_f64_kernel, dim3((unsigned)((hp + 31) / 32), (unsigned)(Np / 32)), dim3(256), 0, st, R, hp, RT, Np,
                       (int)Np, (int)hp);
    if (form == EMCID_SCHUR_XROW) {
        ScopedProf sp(KC_TRSM_DIAG, st);
        GemmShape f{RT, Np, XT, Np, (int)h, (int)Np, (int)Np, 0};
        f.tri = 1; f.pair = 1;       // B(k, n) = XS[n][k] = Xt[k][n], zero for k > n
        launch_gemm_f64<true, false>(f, EpiAxpby{Y2, Np, 1.0, 0.0}, st);
        GemmShape b{Y2, Np, XT, Np, (int)h, (int)Np, (int)Np, 0};
        b.tri = 2; b.pair = 1;       // B(k, n) = XS[k][n] = Xt[n][k], zero for k < n
        launch_gemm_f64<true, true>(b, EpiAxpby{RT, Np, 1.0, 0.0}, st);
    } else if (form == EMCID_SCHUR_FULL_INVERSE) {
        EMCID_TRY(build_full_inverse(LS, Np, Np, invS, full_inv, Y2, y2_doubles, 1, 0, 0, st));
        ScopedProf sp(KC_TRSM_DIAG, st);
        GemmShape f{RT, Np, full_inv, Np, (int)h, (int)Np, (int)Np, 0};
        f.tri = 1; f.pair = 1;       // B(k, n) = XS[n][k], zero for k > n
        launch_gemm_f64<true, true>(f, EpiAxpby{Y2, Np, 1.0, 0.0}, st);
        GemmShape b{Y2, Np, full_inv, Np, (int)h, (int)Np, (int)Np, 0};
        b.tri = 2; b.pair = 1;       // B(k, n) = XS[k][n], zero for k < n
        launch_gemm_f64<true, false>(b, EpiAxpby{RT, Np, 1.0, 0.0}, st);
    } else {
        EMCID_TRY(cholesky_solve_impl(LS, Np, Np, invS, RT, Y2, h, Np, st));
    }
    return EMCID_OK;
}

}  // namespace emcid

using namespace emcid;

extern "C" {

int emcid_assemble_spd_f64(const float* C, int64_t ldc, const double* Kt64, int64_t Np, int64_t d, int64_t ldk, double lam,
                           float cw, double* A, int64_t lda, void* stream) {
    EMCID_CHECK_ARG(C && Kt64 && A && Np > 0 && d > 0);
    const int64_t dp = round_up(d, NB);
    EMCID_CHECK_ARG(lda >= dp && ldk >= dp && ldc >= d && (ldk % 2 == 0) && aligned16(Kt64));
    GemmShape p{Kt64, ldk, Kt64, ldk, (int)dp, (int)dp, (int)Np, 1};
    {
        ScopedProf sp(KC_ASSEMBLE, (hipStream_t)stream);
        launch_gemm_f64<false, false>(p, EpiAssemble{C, ldc, lam, cw, A, lda, (int)d}, (hipStream_t)stream);
    }
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_delta_w_f64(const double* Rt, int64_t ldr, const double* Xt, int64_t ldx, int64_t Np, int64_t h, int64_t d,
                      const float* W0, float* W, int64_t ldw, float* dW, double* U, void* stream) {
    EMCID_CHECK_ARG(Rt && Xt && Np > 0 && h > 0 && d > 0 && ldr % 2 == 0 && ldx % 2 == 0 && aligned16(Rt) && aligned16(Xt));
    EMCID_CHECK_ARG((W == nullptr) || (W0 != nullptr));
    GemmShape p{Rt, ldr, Xt, ldx, (int)h, (int)d, (int)Np, 0};
    {
        ScopedProf sp(KC_DELTA_W, (hipStream_t)stream);
        launch_gemm_f64<false, false>(p, EpiDeltaW{W0, W, ldw, dW, d, U, d}, (hipStream_t)stream);
    }
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_axpy_f32(float* W, const float* dW, int64_t n, void* stream) {
    EMCID_CHECK_ARG(W && dW && n > 0);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpy_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, W, dW, n);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int64_t emcid_edit_workspace_bytes(int64_t N, int64_t d, int64_t h) {
    if (N <= 0 || d <= 0 || h <= 0) return 0;
    return EditWorkspace(N, d, h).total * (int64_t)sizeof(double);
}

static int edit_layer_impl(const float* K, const float* Zc, const float* zs_t, const float* C, int64_t N, int64_t d, int64_t h,
                           double lam, double edit_weight, int layers_left, int64_t n_lo, int64_t n_hi, const float* W0,
                           float* W, double* Xt_out, double* Rt_out, float* dW_out, double* U_out, void* workspace,
                           int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(K && Zc && zs_t && C && N > 0 && d > 0 && h > 0 && layers_left > 0 && workspace && info_dev);
    EMCID_CHECK_ARG(N < (1 << 24) && d <= 32768 && h <= 32768);
    EMCID_CHECK_ARG(0 <= n_lo && n_lo < n_hi && n_hi <= N);
    EMCID_CHECK_ARG((W == nullptr) || (W0 != nullptr));
    EMCID_CHECK_ARG(aligned16(workspace));
    EditWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), " (see emcid_edit_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *A = base + ws.off_A, *L = base + ws.off_L, *inv = base + ws.off_inv;
    double *B = base + ws.off_B, *Y = base + ws.off_Y, *R = base + ws.off_R;
    const float cw = (float)(1.0 - edit_weight);  // torch multiplies the fp32 tensor by the scalar rounded to fp32
    const int64_t rows = n_hi - n_lo;

    launch_prep_kr(K, Zc, zs_t, N, d, h, edit_weight, layers_left, 1.0, B, ws.Np, ws.dp, R, ws.hp, st);
    EMCID_CHECK_LAUNCH();
    EMCID_TRY(emcid_assemble_spd_f64(C, d, B, ws.Np, d, ws.dp, lam, cw, A, ws.dp, stream));
    // only this shard's concept rows go through the triangular solves and the dW contraction
    double* Bs = B + n_lo * ws.dp;
    EMCID_TRY(factor_and_solve(A, L, ws.dp, ws.dp, inv, info_dev, Bs, Y + n_lo * ws.dp, rows, ws.dp, st));
    if (W || dW_out || U_out)
        EMCID_TRY(emcid_delta_w_f64(R + n_lo * ws.hp, ws.hp, Bs, ws.dp, rows, h, d, W0, W, d, dW_out, U_out, stream));
    if (Xt_out)
        hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)rows), dim3(256), 0, st, Bs, ws.dp, Xt_out, d, (int)rows, (int)d);
    if (Rt_out)
        hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)rows), dim3(256), 0, st, R + n_lo * ws.hp, ws.hp, Rt_out, h,
                           (int)rows, (int)h);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_edit_layer_f64(const float* K, const float* Zc, const float* zs_t, const float* C, int64_t N, int64_t d, int64_t h,
                         double lam, double edit_weight, int layers_left, const float* W0, float* W, double* Xt_out,
                         double* Rt_out, float* dW_out, void* workspace, int64_t workspace_bytes, int* info_dev,
                         void* stream) {
    return edit_layer_impl(K, Zc, zs_t, C, N, d, h, lam, edit_weight, layers_left, 0, N, W0, W, Xt_out, Rt_out, dW_out,
                           nullptr, workspace, workspace_bytes, info_dev, stream);
}

int emcid_edit_layer_shard_f64(const float* K, const float* Zc, const float* zs_t, const float* C, int64_t N, int64_t d,
                               int64_t h, double lam, double edit_weight, int layers_left, int64_t n_lo, int64_t n_hi,
                               double* U_partial, double* Xt_out, double* Rt_out, void* workspace, int64_t workspace_bytes,
                               int* info_dev, void* stream) {
    EMCID_CHECK_ARG(U_partial != nullptr);
    return edit_layer_impl(K, Zc, zs_t, C, N, d, h, lam, edit_weight, layers_left, n_lo, n_hi, nullptr, nullptr, Xt_out,
                           Rt_out, nullptr, U_partial, workspace, workspace_bytes, info_dev, stream);
}

int emcid_apply_update_f32(const double* U, const float* W0, float* W, float* dW, int64_t n, void* stream) {
    EMCID_CHECK_ARG(U && n > 0 && (W || dW) && ((W == nullptr) || (W0 != nullptr)));
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(apply_u_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, U, W0, W, dW, n);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- dual (Woodbury) solver ------------------------------------------------------------------------------------- */

int64_t emcid_cov_factor_workspace_bytes(int64_t n_layers, int64_t d) {
    if (n_layers <= 0 || d <= 0) return 0;
    return CovFactorLayout(n_layers, d).total * (int64_t)sizeof(double);
}

int emcid_factor_cov_f64(const float* const* C_host_list, int64_t n_layers, int64_t d, double lam, double edit_weight,
                         void* workspace, int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(C_host_list && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768 && workspace && info_dev);
    EMCID_CHECK_ARG(aligned16(workspace));
    const CovFactorLayout cov(n_layers, d);
    EMCID_CHECK_WORKSPACE(workspace_bytes, cov.total * (int64_t)sizeof(double), " (see emcid_cov_factor_workspace_bytes)");
    const int64_t dp = cov.dp, s_mat = cov.s_mat, s_inv = cov.s_inv;
    // every layer at once (the launches are batched over the layers); X = inv(L) is built per layer by emcid_cov_inverse_f64
    double *Mb = cov.M(workspace, 0), *Lb = cov.L(workspace, 0), *Ib = cov.I(workspace, 0);
    CovPtrs cp;
    for (int i = 0; i < 32; ++i) cp.c[i] = i < n_layers ? C_host_list[i] : nullptr;
    for (int i = 0; i < n_layers; ++i) EMCID_CHECK_ARG(cp.c[i] != nullptr);
    const float cw = (float)(1.0 - edit_weight);
    hipStream_t st = (hipStream_t)stream;
    GraphKey key = make_key(GRAPH_FACTOR_COV, {Mb, info_dev}, {n_layers, d, 0, 0, 0});
    memcpy(&key.num[2], &lam, sizeof(double));
    memcpy(&key.num[3], &cw, sizeof(float));
    for (int i = 0; i < n_layers; ++i)   // every C pointer takes part in the key (6 slots, then folded)
        if (i < 6) key.ptr[2 + i] = cp.c[i]; else key.num[4] = key.num[4] * 1000003 + (int64_t)(uintptr_t)cp.c[i];
    return with_graph(key, st, [&](hipStream_t s) {
        hipLaunchKernelGGL(scale_cov_kernel, dim3((unsigned)dp, (unsigned)n_layers), dim3(256), 0, s, cp, (int)d, (int)dp, lam, cw,
                           Mb, s_mat);
        return cholesky_serial(Mb, Lb, dp, dp, Ib, info_dev, s, (int)n_layers, s_mat, s_inv);
    });
}

/* X_l = inv(L_l) for ONE layer of a factored workspace (needs emcid_factor_cov_f64 earlier on the same stream, or an
 * event dependency on it).  Per layer so that the first edited layer's solve can start while the later layers' inverse
 * factors are still being built underneath it. */
int emcid_cov_inverse_f64(void* cov_factor_ws, int64_t n_layers, int64_t d, int64_t first_layer, int64_t count, void* stream) {
    EMCID_CHECK_ARG(cov_factor_ws && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768 && aligned16(cov_factor_ws));
    EMCID_CHECK_ARG(0 <= first_layer && count > 0 && first_layer + count <= n_layers);
    const CovFactorLayout cov(n_layers, d);
    const int64_t dp = cov.dp;
    double* Mb = cov.M(cov_factor_ws, first_layer);          // consumed by the factorization: scratch now
    const double *Lb = cov.L(cov_factor_ws, first_layer), *Ib = cov.I(cov_factor_ws, first_layer);
    double* Xb = cov.X(cov_factor_ws, first_layer);
    return with_graph(make_key(GRAPH_COV_INVERSE, {Mb, Lb, Ib, Xb}, {dp, count}), (hipStream_t)stream, [&](hipStream_t s) {
        return build_full_inverse(Lb, dp, dp, Ib, Xb, Mb, cov.s_mat, (int)count, cov.s_mat, cov.s_inv, s);   // batched over the range
    });
}

/* ---- a factored workspace at another scale: chol(a M) = sqrt(a) chol(M) ---------------------------------------------------
 * One launch over the three factor regions of every layer: the NB x NB tiles of L on and below the diagonal times sqrt(a), the
 * same tiles of X = inv(L) and the whole block of diagonal-block inverses times 1/sqrt(a).  (A diagonal tile is copied whole:
 * whatever the factorization left above the diagonal inside it travels along, scaled.)  Nothing above the block diagonal is
 * read or written, and the consumed M region is left alone.  Every access is a double2 (128 bits): dp is a multiple of 128 and
 * every region starts on an even number of doubles from the 16-byte aligned base.  src == dst scales in place. */
__global__ __launch_bounds__(256) void cov_factor_rescale_kernel(const double* src, double* dst, int64_t off_L, int64_t off_I,
                                                                 int64_t off_X, int64_t s_mat, int64_t s_inv, int dp, int n_tri,
                                                                 double gain_L, double gain_inv, int with_inverse) {
    const int64_t layer = blockIdx.y;
    const int region = blockIdx.z;            // 0: L, 1: the diagonal-block inverses, 2: X
    if (region == 1) {
        const double2* s = reinterpret_cast<const double2*>(src + off_I + layer * s_inv);
        double2* o = reinterpret_cast<double2*>(dst + off_I + layer * s_inv);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s_inv / 2; i += (int64_t)gridDim.x * 256) {
            double2 v = s[i];
            v.x *= gain_inv;
            v.y *= gain_inv;
            o[i] = v;
        }
        return;
    }
    if (region == 2 && !with_inverse) return;
    const int t = blockIdx.x;                 // tile (I, J), J <= I, of the block lower triangle: t = I (I + 1) / 2 + J
    if (t >= n_tri) return;
    int I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    const int64_t base = (region == 0 ? off_L : off_X) + layer * s_mat + (int64_t)I * NB * dp + (int64_t)J * NB;
    const double g = region == 0 ? gain_L : gain_inv;
    // 128 rows of 64 double2: a wavefront covers one row's 1 KiB
    for (int e = threadIdx.x; e < NB * (NB / 2); e += 256) {
        const int r = e / (NB / 2), c2 = e % (NB / 2);
        const int64_t at = base + (int64_t)r * dp + 2 * c2;
        double2 v = *reinterpret_cast<const double2*>(src + at);
        v.x *= g;
        v.y *= g;
        *reinterpret_cast<double2*>(dst + at) = v;
    }
}

int emcid_cov_factor_rescale_f64(const void* src_ws, void* dst_ws, int64_t workspace_bytes, int64_t n_layers, int64_t d, double a,
                                 int with_inverse, void* stream) {
    EMCID_CHECK_ARG(src_ws && dst_ws && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768);
    EMCID_CHECK_ARG(aligned16(src_ws) && aligned16(dst_ws) && a > 0.0 && a < 1e300);
    const CovFactorLayout cov(n_layers, d);
    EMCID_CHECK_WORKSPACE(workspace_bytes, cov.total * (int64_t)sizeof(double), " (see emcid_cov_factor_workspace_bytes)");
    const int64_t dp = cov.dp, s_inv = cov.s_inv, nt = dp / NB;
    EMCID_CHECK_ARG(s_inv % 2 == 0);
    const double* src = (const double*)src_ws;
    const int n_tri = (int)(nt * (nt + 1) / 2);
    const double root = sqrt(a);
    // grid: x = the tiles of the block lower triangle, y = layer, z = region.  Regions 0 and 2 take one tile per workgroup (all of
    // region 2 leave at once without with_inverse); region 1, the small block of diagonal-block inverses, walks its s_inv / 2
    // double2 with the same n_tri workgroups as a grid-stride loop: one launch for the three regions.
    hipLaunchKernelGGL(cov_factor_rescale_kernel, dim3((unsigned)n_tri, (unsigned)n_layers, 3), dim3(256), 0, (hipStream_t)stream,
                       src, (double*)dst_ws, (int64_t)(cov.L(src, 0) - src), (int64_t)(cov.I(src, 0) - src), (int64_t)(cov.X(src, 0) - src),
                       cov.s_mat, s_inv, (int)dp, n_tri, root, 1.0 / root, with_inverse);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* address of one block of a dual workspace, for the emcid_edit_dual_pt / _yt / _s / _u entries */
static double* dual_block(void* workspace, int64_t N, int64_t d, int64_t h, int64_t DualWorkspace::*off) {
    if (!workspace || N <= 0 || d <= 0 || h <= 0) return nullptr;
    return (double*)workspace + DualWorkspace(N, d, h).*off;
}

int64_t emcid_edit_dual_workspace_bytes(int64_t N, int64_t d, int64_t h) {
    if (N <= 0 || d <= 0 || h <= 0) return 0;
    return DualWorkspace(N, d, h).total * (int64_t)sizeof(double);
}

/* any block of a dual workspace by name, with its length (tests read the intermediates of the chain through this) */
double* emcid_edit_dual_block(void* workspace, int64_t N, int64_t d, int64_t h, int which, int64_t* doubles_out) {
    if (doubles_out) *doubles_out = -1;
    int64_t off = 0, n = 0;
    if (!workspace || N <= 0 || d <= 0 || h <= 0 || !DualWorkspace(N, d, h).block(which, &off, &n)) return nullptr;
    if (doubles_out) *doubles_out = n;
    return (double*)workspace + off;
}

/* how stage 2 of the apply-only form will solve Z = S^-1 Rt for these dimensions: EMCID_SCHUR_* (host only, launches nothing) */
int emcid_edit_dual_schur_form(int64_t N, int64_t d, int64_t h) {
    if (N <= 0 || d <= 0 || h <= 0) return -1;
    const DualWorkspace ws(N, d, h);
    return schur_rhs_form(ws.Np, cholesky_takes_shadow(ws.Np), true, ws.y2_doubles());
}

/* what stage 1 of the adj_k form and of the apply-only form ask of the same argument list (a macro: the message names the entry) */
#define EMCID_CHECK_DUAL_STAGE1_ARGS()                                                                            \
    EMCID_CHECK_ARG(K && Zc && zs_t && N > 0 && d > 0 && h > 0 && layers_left > 0 && cov_factor_ws && workspace); \
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers && 0 <= n_lo && n_lo < n_hi && n_hi <= N);         \
    EMCID_CHECK_ARG(lam_ratio > 0.0 && lam_ratio < 1e300)

/* stage 1: Kt64 = s*K, Rt, and the shard's rows of Pt = Kt64 M^-1 (into Pt_rows_out if given, else only the workspace) */
int emcid_edit_dual_stage1_f64(const float* K, const float* Zc, const float* zs_t, int64_t N, int64_t d, int64_t h,
                               double edit_weight, int layers_left, double lam_ratio, const void* cov_factor_ws, int64_t n_layers,
                               int64_t layer_index, int64_t n_lo, int64_t n_hi, int use_inverse, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    EMCID_CHECK_DUAL_STAGE1_ARGS();
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Kt = base + ws.off_K, *Pt = base + ws.off_P, *Y = base + ws.off_Y, *R = base + ws.off_R;
    const int64_t dp = ws.dp;
    const CovFactorLayout cov(n_layers, d);
    const double *Lb = cov.L(cov_factor_ws, layer_index), *Ib = cov.I(cov_factor_ws, layer_index);
    launch_prep_kr(K, Zc, zs_t, N, d, h, edit_weight, layers_left, 1.0 / sqrt(lam_ratio), Kt, ws.Np, dp, R, ws.hp, st);
    const int64_t rows = n_hi - n_lo;
    if (use_inverse) {
        // Pt = (Kt X^T) X : both triangular solves against M = L L^T are GEMMs against the explicit X = inv(L)
        const double* Xb = cov.X(cov_factor_ws, layer_index);
        apply_inverse_forward(Xb, dp, Kt + n_lo * dp, Y + n_lo * dp, (int)rows, st, base + ws.off_SK);
        apply_inverse_backward(Xb, dp, Y + n_lo * dp, (int)rows, (int)dp, Pt + n_lo * dp, dp, st, base + ws.off_SK);
        EMCID_CHECK_LAUNCH();
        return EMCID_OK;
    }
    if (hipMemcpyAsync(Pt + n_lo * dp, Kt + n_lo * dp, rows * dp * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(EMCID_ERR_HIP, __func__, "hipMemcpyAsync");
    return with_graph(make_key(GRAPH_DUAL_STAGE1, {Lb, Ib, Pt + n_lo * dp, Y + n_lo * dp}, {dp, rows}), st, [&](hipStream_t q) {
        return cholesky_solve_impl(Lb, dp, dp, Ib, Pt + n_lo * dp, Y + n_lo * dp, rows, dp, q);
    });
}

/* pointer to the Pt stack [Np, dp] inside a dual workspace (multi-GPU: ranks all-gather their row blocks in place) */
double* emcid_edit_dual_pt(void* workspace, int64_t N, int64_t d, int64_t h) { return dual_block(workspace, N, d, h, &DualWorkspace::off_P); }

/* stage 2 (needs ALL rows of Pt): S = I + Pt Kt^T, S = L_S L_S^T, adj_k = (S^-1 Pt)^T  [d, Np], U = Rt^T Xt, W = W0 + float(U) */
int emcid_edit_dual_stage2_f64(int64_t N, int64_t d, int64_t h, double lam_ratio, const float* W0, float* W, double* adjk_out, double* Rt_out,
                               float* dW_out, void* workspace, int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(N > 0 && d > 0 && h > 0 && workspace && info_dev && ((W == nullptr) || (W0 != nullptr)));
    EMCID_CHECK_ARG(lam_ratio > 0.0 && lam_ratio < 1e300);
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Kt = base + ws.off_K, *Pt = base + ws.off_P, *R = base + ws.off_R, *S = base + ws.off_S, *LS = base + ws.off_LS;
    double *invS = base + ws.off_invS, *PT = base + ws.off_PT, *Y2 = base + ws.off_Y2;
    const int64_t dp = ws.dp, Np = ws.Np;
    EMCID_TRY(with_graph(make_key(GRAPH_DUAL_STAGE2,{Kt, Pt, S, LS, invS, PT, Y2, info_dev}, {dp, Np, N}), st, [&](hipStream_t q) {
        if (Np > N)   // rows of the padding concepts: zero (their Kt rows are zero, so S gets identity rows there)
            hipLaunchKernelGGL(zero_f64_kernel, dim3(256), dim3(256), 0, q, Pt + N * dp, (Np - N) * dp);
        assemble_dual_system(Pt, Kt, dp, S, (int)Np, q, base + ws.off_SK);
        EMCID_TRY(cholesky_impl(S, LS, Np, Np, invS, info_dev, q));
        hipLaunchKernelGGL(transpose_f64_kernel, dim3((unsigned)(dp / 32), (unsigned)(Np / 32)), dim3(256), 0, q, Pt, dp, PT, Np,
                           (int)Np, (int)dp);
        return cholesky_solve_impl(LS, Np, Np, invS, PT, Y2, dp, Np, q);   // PT := PT S^-1  ->  adj_k padded [dp, Np]
    }));
    if (W || dW_out) {
        ScopedProf sp(KC_DELTA_W, st);
        GemmShape g{R, ws.hp, PT, Np, (int)h, (int)d, (int)Np, 0};
        launch_gemm_f64<false, true>(g, EpiDeltaW{W0, W, d, dW_out, d, nullptr, d}, st);
    }
    // the workspace holds sqrt(lam_ratio) * adj_k and Rt / sqrt(lam_ratio) (stage 1's gain): the caller gets both in its own scale
    const double root = sqrt(lam_ratio);
    if (adjk_out)
        hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)d), dim3(256), 0, st, PT, Np, adjk_out, N, (int)d, (int)N, 1.0 / root);
    if (Rt_out) hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)N), dim3(256), 0, st, R, ws.hp, Rt_out, h, (int)N, (int)h, root);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- dual solver, apply-only form: adj_k is never formed -----------------------------------------------------------
 * With M = L L^T:  Yt = Kt64 L^-T,  S = I + Yt Yt^T,  Z = S^-1 Rt,  U = Rt^T Xt = (Z^T Yt) L^-1,  W = W0 + float(U).
 * One forward solve on the N concept rows, a true SYRK, the N x N Cholesky, two solves with only h right-hand sides,
 * one GEMM and one backward solve on h rows.  Same algebra as stage1 + stage2 by associativity. */
int emcid_edit_dual_apply_stage1_f64(const float* K, const float* Zc, const float* zs_t, int64_t N, int64_t d, int64_t h,
                                     double edit_weight, int layers_left, double lam_ratio, const void* cov_factor_ws, int64_t n_layers,
                                     int64_t layer_index, int64_t n_lo, int64_t n_hi, int use_inverse, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    EMCID_CHECK_DUAL_STAGE1_ARGS();
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Kt = base + ws.off_K, *Bs = base + ws.off_P, *Yt = base + ws.off_Y, *R = base + ws.off_R;
    const int64_t dp = ws.dp;
    const CovFactorLayout cov(n_layers, d);
    const double *Lb = cov.L(cov_factor_ws, layer_index), *Ib = cov.I(cov_factor_ws, layer_index);
    launch_prep_kr(K, Zc, zs_t, N, d, h, edit_weight, layers_left, 1.0 / sqrt(lam_ratio), Kt, ws.Np, dp, R, ws.hp, st);
    const int64_t rows = n_hi - n_lo;
    if (use_inverse) {
        // the whole concept range: run over the Np padded rows (Kt's padding rows are zero, so are the products) — every
        // 128-row tile then lies inside the operand and takes the interior fast path of the stream-K K loop
        const int64_t gemm_rows = (n_lo == 0 && n_hi == N) ? ws.Np : rows;
        apply_inverse_forward(cov.X(cov_factor_ws, layer_index), dp, Kt + n_lo * dp, Yt + n_lo * dp, (int)gemm_rows, st,
                              base + ws.off_SK);
        // stage 1 leaves the padding rows [N, Np) of Yt zero (the later stages rely on it): the full-range GEMM has just produced
        // them; a partial range (row-sharded callers) zeroes them here
        if (gemm_rows != ws.Np && ws.Np > N)
            hipLaunchKernelGGL(zero_f64_kernel, dim3(256), dim3(256), 0, st, Yt + N * dp, (ws.Np - N) * dp);
        EMCID_CHECK_LAUNCH();
        return EMCID_OK;
    }
    if (ws.Np > N) hipLaunchKernelGGL(zero_f64_kernel, dim3(256), dim3(256), 0, st, Yt + N * dp, (ws.Np - N) * dp);
    if (hipMemcpyAsync(Bs + n_lo * dp, Kt + n_lo * dp, rows * dp * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(EMCID_ERR_HIP, __func__, "hipMemcpyAsync");
    return with_graph(make_key(GRAPH_APPLY_STAGE1,{Lb, Ib, Bs + n_lo * dp, Yt + n_lo * dp}, {dp, rows}), st, [&](hipStream_t q) {
        trsm_forward(Lb, dp, dp, OB, Ib, Bs + n_lo * dp, dp, Yt + n_lo * dp, dp, (int)rows, q);
        return check_launch("emcid_edit_dual_apply_stage1_f64");
    });
}

/* address of the Yt stack [Np, dp] inside a dual workspace (multi-GPU: ranks all-gather their row blocks there) */
double* emcid_edit_dual_yt(void* workspace, int64_t N, int64_t d, int64_t h) { return dual_block(workspace, N, d, h, &DualWorkspace::off_Y); }

/* The first part of stage 2 on its own: S = I + Yt Yt^T.  A caller that wants to start other work exactly when the
 * latency-bound Cholesky of S begins (the engine builds the next layer's inverse factor on a second stream then) calls
 * this, records its event, and passes assembled = 1 to stage 2. */
int emcid_edit_dual_apply_assemble_f64(int64_t N, int64_t d, int64_t h, void* workspace, int64_t workspace_bytes, void* stream) {
    EMCID_CHECK_ARG(N > 0 && d > 0 && h > 0 && workspace);
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Yt = base + ws.off_Y, *S = base + ws.off_S;
    const int64_t dp = ws.dp, Np = ws.Np;
    assemble_dual_system(Yt, Yt, dp, S, (int)Np, st, base + ws.off_SK);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_edit_dual_apply_stage2_f64(int64_t N, int64_t d, int64_t h, const void* cov_factor_ws, int64_t n_layers,
                                     int64_t layer_index, int use_inverse, int assembled, const float* W0, float* W,
                                     float* dW_out, void* workspace, int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(N > 0 && d > 0 && h > 0 && workspace && info_dev && cov_factor_ws && ((W == nullptr) || (W0 != nullptr)));
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers && (W || dW_out));
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Yt = base + ws.off_Y, *R = base + ws.off_R, *S = base + ws.off_S, *LS = base + ws.off_LS, *invS = base + ws.off_invS;
    double *RT = base + ws.off_PT, *Y2 = base + ws.off_Y2, *V = base + ws.off_V, *U = base + ws.off_U;
    const int64_t dp = ws.dp, Np = ws.Np, hp = ws.hp;
    const CovFactorLayout cov(n_layers, d);
    const double *Lb = cov.L(cov_factor_ws, layer_index), *Ib = cov.I(cov_factor_ws, layer_index);
    // P = Yt X rides in the Cholesky's leaf launches (ShadowJob) when X is explicit and the fused schedule runs: then
    // U = Z^T P is one GEMM and the GEMM against the triangle after the N x N solve (U = (Z^T Yt) X) disappears from the chain
    static const int shadow_env = env_flag("EMCID_SHADOW_P", 1);      // 0: never, 1: when it fits under the leaves, 2: always
    bool shadow = shadow_env && use_inverse && cholesky_takes_shadow(Np);
    if (shadow && shadow_env == 1) {
        // The product only pays while a launch's shadow tiles finish about when its leaf does (~36 us).  Measured on MI355X
        // (scripts/step_stamps.py): a tile pair's slice costs ~9 us + 1.5 us per 16-deep K step, one workgroup per compute unit.
        // SD dims, N = 1000: 25 steps, 192 workgroups -> 46 us; SDXL TE2 (d = 5120) at N = 1000: 41 steps in two rounds -> no.
        const int64_t ntl = (dp + SH_BN - 1) / SH_BN, nb = Np / NB;
        const int64_t steps = ((ntl + 1) * (SH_BN / 16) + nb - 1) / nb;
        const int64_t wgs = ((Np + SH_BM - 1) / SH_BM) * ((ntl + 1) / 2), rounds = (wgs + 239) / 240;
        shadow = rounds * (9.0 + 1.5 * (double)steps) <= 50.0;
    }
    double* P = base + ws.off_P;
    const double* X = use_inverse ? cov.X(cov_factor_ws, layer_index) : nullptr;
    // Few concepts (a 100-concept edit: Np = 128, no chain of leaves to ride in): U = Z^T (Yt X) with the triangle multiplied on the
    // Np-row side as a launch of its own, instead of U = (Z^T Yt) X on the h-row side — 128 rows against 768 at SD dims
    // (61 + ~15 us instead of ~20 + 155 per layer).
    const bool p_first = !shadow && use_inverse && Np < h;
    const bool xrow = cholesky_takes_shadow(Np);       // (= the fused leaf / spine schedule runs)
    double *XT = base + ws.off_XT, *TT = base + ws.off_TT;
    EMCID_TRY(with_graph(make_key(GRAPH_APPLY_STAGE2, {Yt, R, S, LS, RT, V, U, info_dev},
                                  {dp, Np, N, hp, (int64_t)(uintptr_t)Lb,
                                   use_inverse + 2 * (assembled != 0) + 4 * (int)shadow + 8 * h + ((int64_t)p_first << 31) + ((int64_t)xrow << 30) + (d << 32)}),
                         st,
                         [&](hipStream_t q) {
        if (!assembled) {
            assemble_dual_system(Yt, Yt, dp, S, (int)Np, q, base + ws.off_SK);      // S = I + Yt Yt^T (lower tiles)
        }
        if (p_first) apply_inverse_backward(X, dp, Yt, (int)Np, (int)dp, P, dp, q, base + ws.off_SK);       // P = Yt X
        ShadowJob job{Yt, dp, X, dp, P, dp, (int)Np, (int)dp, (int)dp, 0, nullptr, 0, 0, 0};
        job.wgs = (int)((Np + SH_BM - 1) / SH_BM) * (int)(((dp + SH_BN - 1) / SH_BN + 1) / 2);
        // XS = inv(LS) rides in the factorization's launches (XrowJob), transposed
        const XrowJob xj{XT, Np, TT};
        EMCID_TRY(cholesky_impl(S, LS, Np, Np, invS, info_dev, q, shadow ? &job : nullptr, xrow ? &xj : nullptr));
        // RT[h, Np] = Rt^T ; Z^T = RT S^-1 (two solves with h rows)
        EMCID_TRY(solve_schur_rhs(R, hp, h, Np, LS, invS, xrow ? XT : nullptr, S, RT, Y2, ws.y2_doubles(), q));
        if (!shadow && !p_first) {
            ScopedProf sp(KC_DELTA_W, q);       // V[h, dp] = Z^T Yt
            GemmShape g{RT, Np, Yt, dp, (int)h, (int)dp, (int)Np, 0};
            launch_gemm_f64<true, false>(g, EpiAxpby{V, dp, 1.0, 0.0}, q);
        }
        if (!use_inverse) trsm_backward(Lb, dp, dp, OB, Ib, V, dp, U, dp, (int)h, q);   // U L = V by block substitution
        return check_launch("emcid_edit_dual_apply_stage2_f64");
    }));
    if (shadow || p_first) {
        // U = Z^T P straight into the weights: W = W0 + float(U), dW = float(U) in the GEMM's epilogue (outside the cached graph:
        // W0 / W / dW are the caller's tensors and change from layer to layer and call to call)
        ScopedProf sp(KC_DELTA_W, st);
        GemmShape g{RT, Np, P, dp, (int)h, (int)d, (int)Np, 0};
        launch_gemm_f64<true, false>(g, EpiDeltaW{W0, W, d, dW_out, d, nullptr, 0}, st, -1);      // the launcher's choice: 32 x 64 tiles
        EMCID_CHECK_LAUNCH();
        return EMCID_OK;
    }
    if (use_inverse)   // U = V inv(L)  (V's padding columns are zero: Kt's are, X is the identity there)
        apply_inverse_backward(X, dp, V, (int)h, (int)dp, U, dp, st, base + ws.off_SK);
    hipLaunchKernelGGL(apply_u2d_kernel, dim3((unsigned)h), dim3(256), 0, st, U, dp, W0, W, dW_out, (int)d);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- dual solver, apply-only form, COLUMN-SHARDED over ranks (multi-GPU) -----------------------------------
 * The d columns of Yt = Kt64 X^T are dealt to the ranks in 128-wide tiles (`tiles`: this rank's tile indices, ascending).
 * With Yc = the rank's columns of Yt:
 *     S = I + sum_ranks Yc Yc^T        (one all-reduce of the N x N partial sums — the only coupling of the concepts)
 *     V[:, mine] = Z^T Yc,  Z = S^-1 Rt (every rank factors S itself: d^3-free, latency-bound, 0.5 ms)
 *     U = V X = sum_ranks V[:, mine] X[mine, :]      (one all-reduce of the h x d partial sums)
 * so a rank's GEMM work is 1/world of the layer's and nothing but S and U crosses the links.  Needs X = inv(L) of the layer
 * (emcid_cov_inverse_f64).  stage 1 leaves the partial S (no identity) at emcid_edit_dual_s(); stage 2 expects the SUMMED S
 * there and leaves the partial U (leading dimension dp = d rounded up to 128) at emcid_edit_dual_u(). */
__global__ __launch_bounds__(256) void add_identity_f64_kernel(double* __restrict__ S, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) S[(int64_t)i * n + i] += 1.0;
}

static int check_tiles(const int* tiles, int n_tiles, int64_t dp) {
    if (!tiles || n_tiles <= 0 || n_tiles > 256) return 0;
    for (int i = 0; i < n_tiles; ++i)
        if (tiles[i] < 0 || (int64_t)tiles[i] * NB >= dp || (i > 0 && tiles[i] <= tiles[i - 1])) return 0;
    return 1;
}

int emcid_edit_dual_cols_stage1_f64(const float* K, const float* Zc, const float* zs_t, int64_t N, int64_t d, int64_t h,
                                    double edit_weight, int layers_left, double lam_ratio, const void* cov_factor_ws, int64_t n_layers,
                                    int64_t layer_index, const int* tiles_host, int n_tiles, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    EMCID_CHECK_ARG(K && Zc && zs_t && N > 0 && d > 0 && h > 0 && layers_left > 0 && cov_factor_ws && workspace);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers && lam_ratio > 0.0 && lam_ratio < 1e300);
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_ARG(check_tiles(tiles_host, n_tiles, ws.dp));
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Kt = base + ws.off_K, *Yc = base + ws.off_Y, *R = base + ws.off_R, *S = base + ws.off_S, *sk = base + ws.off_SK;
    const int64_t dp = ws.dp, Np = ws.Np;
    const double* X = CovFactorLayout(n_layers, d).X(cov_factor_ws, layer_index);
    launch_prep_kr(K, Zc, zs_t, N, d, h, edit_weight, layers_left, 1.0 / sqrt(lam_ratio), Kt, Np, dp, R, ws.hp, st);
    for (int i = 0; i < n_tiles; ++i) {        // Yc[:, 128 i : 128 i + 128] = Kt[:, 0 : kd] X[128 t : 128 t + 128, 0 : kd]^T,  kd = 128 (t + 1)
        const int64_t t = tiles_host[i], kd = (t + 1) * NB;
        ScopedProf sp(KC_INV_APPLY, st);
        GemmShape g{Kt, dp, X + t * NB * dp, dp, (int)Np, NB, (int)kd, 0};
        if (!launch_gemm_f64_streamk2<true, true>(g, EpiAxpby{Yc + (int64_t)i * NB, dp, 1.0, 0.0}, st, kStreamKWgs, sk))
            return fail(EMCID_ERR_BAD_ARG, __func__, "more output tiles than stream-K ticket counters");
    }
    {   // partial S = Yc Yc^T on the lower 128-tiles, K = 128 n_tiles deep
        ScopedProf sp(KC_ASSEMBLE, st);
        GemmShape g{Yc, dp, Yc, dp, (int)Np, (int)Np, n_tiles * NB, 1};
        if (!launch_gemm_f64_streamk2<true, true>(g, EpiAxpby{S, Np, 1.0, 0.0}, st, kStreamKWgs, sk, 0.0))
            return fail(EMCID_ERR_BAD_ARG, __func__, "more output tiles than stream-K ticket counters");
    }
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

double* emcid_edit_dual_s(void* workspace, int64_t N, int64_t d, int64_t h) { return dual_block(workspace, N, d, h, &DualWorkspace::off_S); }

double* emcid_edit_dual_u(void* workspace, int64_t N, int64_t d, int64_t h) { return dual_block(workspace, N, d, h, &DualWorkspace::off_U); }

int emcid_edit_dual_cols_stage2_f64(int64_t N, int64_t d, int64_t h, const void* cov_factor_ws, int64_t n_layers,
                                    int64_t layer_index, const int* tiles_host, int n_tiles, void* workspace,
                                    int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(N > 0 && d > 0 && h > 0 && workspace && info_dev && cov_factor_ws);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers);
    DualWorkspace ws(N, d, h);
    EMCID_CHECK_ARG(check_tiles(tiles_host, n_tiles, ws.dp));
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Yc = base + ws.off_Y, *R = base + ws.off_R, *S = base + ws.off_S, *LS = base + ws.off_LS, *invS = base + ws.off_invS;
    double *RT = base + ws.off_PT, *Y2 = base + ws.off_Y2, *V = base + ws.off_V, *U = base + ws.off_U;
    const int64_t dp = ws.dp, Np = ws.Np, hp = ws.hp;
    // (solve_schur_rhs refuses the same, but only behind add_identity and the factorization: outside a graph capture S would
    // already be rewritten.  A refused call launches nothing.)
    if (ws.y2_doubles() < hp * Np) return fail(EMCID_ERR_WORKSPACE, __func__, "RT / Y2 hold fewer than h rows of Np (h > d rounded up to 128)");
    const double* X = CovFactorLayout(n_layers, d).X(cov_factor_ws, layer_index);
    const int w = n_tiles * NB;
    const bool xrow = cholesky_takes_shadow(Np);
    EMCID_TRY(with_graph(make_key(GRAPH_COLS_STAGE2,{Yc, R, S, LS, RT, V, U, info_dev}, {dp, Np, N, hp, (int64_t)w + ((int64_t)xrow << 40)}), st, [&](hipStream_t q) {
        hipLaunchKernelGGL(add_identity_f64_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, q, S, (int)Np);
        const XrowJob xj{base + ws.off_XT, Np, base + ws.off_TT};
        EMCID_TRY(cholesky_impl(S, LS, Np, Np, invS, info_dev, q, nullptr, xrow ? &xj : nullptr));
        // RT := Z^T, against the inverse that rode in the factorization or by substitution
        EMCID_TRY(solve_schur_rhs(R, hp, h, Np, LS, invS, xrow ? xj.Xt : nullptr, nullptr, RT, Y2, ws.y2_doubles(), q));
        {
            ScopedProf sp(KC_DELTA_W, q);       // V[h, w] = Z^T Yc
            GemmShape g{RT, Np, Yc, dp, (int)h, w, (int)Np, 0};
            launch_gemm_f64<true, false>(g, EpiAxpby{V, dp, 1.0, 0.0}, q);
        }
        hipLaunchKernelGGL(zero2d_f64_kernel, dim3((unsigned)h, 1u), dim3(256), 0, q, U, dp, (int64_t)0, (int)dp);
        return check_launch("emcid_edit_dual_cols_stage2_f64");
    }));
    for (int i = 0; i < n_tiles; ++i) {        // U[:, 0 : kd] += V[:, 128 i : 128 i + 128] X[128 t : 128 t + 128, 0 : kd]
        const int64_t t = tiles_host[i], kd = (t + 1) * NB;
        ScopedProf sp(KC_INV_APPLY, st);
        GemmShape g{V + (int64_t)i * NB, dp, X + t * NB * dp, dp, (int)h, (int)kd, NB, 0};
        launch_gemm_f64<true, false>(g, EpiAxpby{U, dp, 1.0, 1.0}, st);
    }
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* W = W0 + float(U) (optional), dW = float(U) (optional) for U [h][ldu] f64 with ldu >= d (the padded partial sums above) */
int emcid_apply_update2d_f32(const double* U, int64_t ldu, const float* W0, float* W, float* dW, int64_t h, int64_t d, void* stream) {
    EMCID_CHECK_ARG(U && h > 0 && d > 0 && ldu >= d && (W || dW) && ((W == nullptr) || (W0 != nullptr)));
    hipLaunchKernelGGL(apply_u2d_kernel, dim3((unsigned)h), dim3(256), 0, (hipStream_t)stream, U, ldu, W0, W, dW, (int)d);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

}  // extern "C"
