// Edit sessions on the apply-only dual form (edit_solve.hip): a layer keeps the keys of earlier steps in factor coordinates, and a
// step is a bordered Cholesky behind them.  Preserve (an edit's rows), retain (rows with a zero residual), release (rows leave,
// the rest is rebuilt), the per-step readout, the fold of a full preserved set into a covariance factor of its own, and the release of
// rows a fold has taken (the same rows subtracted from the folded system, all layers refactored in one batched chain).
#include "spd_solve.h"

namespace emcid {

// Kt64[n][j] = double(K[n][j]) * s * g alone (zero padded to [Np][dp]): a retained key (emcid_session_retain_f64) has no
// residual side; the conversion is prep_kr_kernel's (edit_solve.hip), operation for operation
__global__ __launch_bounds__(256) void prep_k_kernel(const float* __restrict__ K, int N, int d, double s, double* __restrict__ Kt64,
                                                      int dp, double g) {
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < dp; j += 256) {
        double v = 0.0;
        if (n < N && j < d) v = (double)K[(int64_t)n * d + j] * s * g;
        Kt64[(int64_t)n * dp + j] = v;
    }
}

// The readout of a preserve step (emcid_session_step_norms_f64): one wave per output, four outputs per workgroup.
//   o <  M              drift[o]        = || ZT[0:h, o] ||_2          (ZT = [Zp^T | Zk^T] [h][ldz]: column o, strided by ldz)
//   M <= o < M + N      left[o - M]     = || ZT[0:h, o] ||_2
//   M + N <= o          resid[o - M - N] = || Rt[o - M - N, 0:h] ||_2  (Rt [N][ldr])
__global__ __launch_bounds__(256) void step_norms_kernel(const double* __restrict__ ZT, int64_t ldz, const double* __restrict__ Rt,
                                                          int64_t ldr, int h, int M, int N, double* __restrict__ drift,
                                                          double* __restrict__ left, double* __restrict__ resid) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= M + 2 * N) return;       // (whole waves leave: no lane of a wave that stays is missing from the shuffles)
    double s = 0.0;
    if (o < M + N) {
        for (int i = lane; i < h; i += 64) {
            const double v = ZT[(int64_t)i * ldz + o];
            s += v * v;
        }
    } else {
        const double* r = Rt + (int64_t)(o - M - N) * ldr;
        for (int i = lane; i < h; i += 64) s += r[i] * r[i];
    }
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) {
        if (o < M) drift[o] = sqrt(s);
        else if (o < M + N) left[o - M] = sqrt(s);
        else resid[o - M - N] = sqrt(s);
    }
}

// dst[j][0:dp] = src[idx[j]][0:dp] for j < n, zero for the padding rows n <= j < gridDim.x (emcid_session_release_f64: the kept rows
// of Yp, gathered through the workspace because they overlap their destination).  One workgroup per row, double2; src, dst 16-byte
// aligned, lds_ and dp even.  An index outside [0, rows) reads nothing: the row is zeroed.
__global__ __launch_bounds__(256) void gather_rows_f64_kernel(const double* __restrict__ src, int64_t lds_, const int32_t* __restrict__ idx,
                                                               int n, int rows, double* __restrict__ dst, int dp) {
    const int j = blockIdx.x;
    const int r = j < n ? idx[j] : -1;
    const double2* s = r >= 0 && r < rows ? reinterpret_cast<const double2*>(src + (int64_t)r * lds_) : nullptr;
    double2* o = reinterpret_cast<double2*>(dst + (int64_t)j * dp);
    for (int c = threadIdx.x; c < dp / 2; c += 256) o[c] = s ? s[c] : make_double2(0.0, 0.0);
}

// dst[j][0:dp] = factors[first + j] * src[first + j][0:dp] for j < n, zero for the padding rows n <= j < gridDim.x
// (emcid_session_rescale_f64: the rows behind `first`, scaled through the workspace because with src == Yp they overlap their
// destination).  One workgroup per row, double2, one multiply per element; src, dst 16-byte aligned, lds_ and dp even.
__global__ __launch_bounds__(256) void scale_rows_f64_kernel(const double* __restrict__ src, int64_t lds_, const double* __restrict__ factors,
                                                              int first, int n, double* __restrict__ dst, int dp) {
    const int j = blockIdx.x;
    const double f = j < n ? factors[first + j] : 0.0;
    const double2* s = j < n ? reinterpret_cast<const double2*>(src + (int64_t)(first + j) * lds_) : nullptr;
    double2* o = reinterpret_cast<double2*>(dst + (int64_t)j * dp);
    for (int c = threadIdx.x; c < dp / 2; c += 256) {
        double2 v = make_double2(0.0, 0.0);
        if (s) {
            v = s[c];
            v.x *= f;
            v.y *= f;
        }
        o[c] = v;
    }
}

// ---- dual solver with a preserved key set (edit sessions) ---------------------------------------------------------------------
// State of a layer: Yp [M, dp] (the Yt rows of every earlier step), Lp = chol(I + Yp Yp^T) [M, M], and the inverses of Lp's
// 128 x 128 diagonal tiles (they keep the two solves against Lp GEMM-shaped).  A step appends N rows to all three.

// Inverse of one diagonal tile of Lp, extended by the rows a step appended: column j of inv(L) only depends on column j
// (x_ij = (delta_ij - sum_{j <= k < i} L_ik x_kj) / L_ii), so 16 columns go to one wave — 4 lanes per column share the k sum —
// and the rows [0, r0) the state already holds are read back, not recomputed.  grid (tiles touched by rows [M, MN), 8).
__global__ __launch_bounds__(64) void tile_inverse_extend_kernel(const double* __restrict__ Lp, int64_t ldl, double* __restrict__ T,
                                                                  int M, int MN) {
    const int J = M / NB + blockIdx.x, c = J * NB;
    const int r0 = M > c ? M - c : 0, r1 = (MN - c) < NB ? (MN - c) : NB;
    const int lane = threadIdx.x, jl = lane & 15, part = lane >> 4, j = blockIdx.y * 16 + jl;
    __shared__ double Xs[NB][17];
    double* Tt = T + (int64_t)J * NB * NB;
    for (int i = part; i < r0; i += 4) Xs[i][jl] = Tt[i * NB + j];
    __syncthreads();
    const double* Lt = Lp + (int64_t)c * ldl + c;
    for (int i = r0; i < r1; ++i) {
        const double* Li = Lt + (int64_t)i * ldl;
        double s = 0.0;
        for (int k = j + part; k < i; k += 4) s += Li[k] * Xs[k][jl];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const double x = j > i ? 0.0 : ((j == i ? 1.0 : 0.0) - s) / Li[i];
        if (part == 0) {
            Xs[i][jl] = x;
            Tt[i * NB + j] = x;
        }
        __syncthreads();
    }
}

// Lp[M + i][M + j] = LS[i][j] on and below the diagonal, zero above it (i, j < N)
__global__ __launch_bounds__(256) void append_factor_kernel(const double* __restrict__ LS, int64_t lds_, double* __restrict__ Lp,
                                                             int64_t ldl, int M, int N) {
    const int i = blockIdx.x;
    double* row = Lp + (int64_t)(M + i) * ldl + M;
    for (int j = threadIdx.x; j < N; j += 256) row[j] = j <= i ? LS[(int64_t)i * lds_ + j] : 0.0;
}

// the blocks of a workspace that the key half of a step works on (session_append_rows)
struct KeyHalf {
    double *Yt, *S, *LS, *invS, *XT, *TT, *B;
    int64_t dp, Np, cp;
};

struct PreserveWorkspace {
    DualWorkspace dual;
    int64_t cp, off_B, off_ZT, off_G, total;   // doubles
    PreserveWorkspace(int64_t N, int64_t d, int64_t h, int64_t capacity) : dual(N, d, h) {
        cp = round_up(capacity, NB);
        int64_t o = dual.total;
        off_B = o; o += dual.Np * cp;        // B = Yk Yp^T, consumed by the forward solve
        off_ZT = o; o += dual.hp * cp;       // [Zp^T | Zk^T]
        off_G = o; o += dual.hp * cp;        // -(Zk^T Lkp), consumed by the backward solve
        total = o;
    }
    KeyHalf key_half(double* base) const {
        return {base + dual.off_Y, base + dual.off_S, base + dual.off_LS, base + dual.off_invS, base + dual.off_XT, base + dual.off_TT,
                base + off_B, dual.dp, dual.Np, cp};
    }
};

// workspace of emcid_session_retain_f64: the key half of a PreserveWorkspace (no Rt, RT, Y2, V, U, ZT, G)
struct RetainWorkspace {
    int64_t Np, dp, cp;
    int64_t off_K, off_Y, off_S, off_LS, off_invS, off_SK, off_XT, off_TT, off_B, total;   // doubles
    RetainWorkspace(int64_t N, int64_t d, int64_t capacity) {
        Np = round_up(N, NB);
        dp = round_up(d, NB);
        cp = round_up(capacity, NB);
        int64_t o = 0;
        off_K = o; o += Np * dp;
        off_Y = o; o += Np * dp;
        off_S = o; o += Np * Np;
        off_LS = o; o += Np * Np;
        off_invS = o; o += inv_doubles(Np);
        off_SK = o; o += streamk_workspace_doubles(kStreamKWgs);
        off_XT = o; o += Np * Np;
        off_TT = o; o += Np * NB;
        off_B = o; o += Np * cp;
        total = o;
    }
    KeyHalf key_half(double* base) const {
        return {base + off_Y, base + off_S, base + off_LS, base + off_invS, base + off_XT, base + off_TT, base + off_B, dp, Np, cp};
    }
};

// what the session entries ask of the caller's state (Yp, Lp, tile inverses) for N rows behind row M
static bool session_state_ok(int64_t M, int64_t N, int64_t d, const double* Yp, int64_t ldy, const double* Lp, int64_t ldl,
                             const double* tile_inv, int64_t capacity) {
    return M >= 0 && M + N <= capacity && capacity < (int64_t)1 << 30 && ldy >= round_up(d, NB) && ldy % 2 == 0 && ldl >= capacity &&
           ldl % 2 == 0 && aligned16(Yp) && aligned16(Lp) && aligned16(tile_inv);
}

// The key half of a step behind row M, from N rows that already are in factor coordinates (k.Yt [Np][dp]): the copy into Yp,
// B = Yk Yp^T, Lkp = B Lp^-T, T = I + Yk Yk^T - Lkp Lkp^T, its Cholesky (the explicit inverse XS = inv(LS) riding in the
// factorization's launches as an XrowJob, transposed, when the fused schedule runs), the append and the tile inverses.  A preserve
// step, a retain list and a release all run it.
static int session_append_rows(const KeyHalf& k, int64_t N, double* Yp, int64_t ldy, double* Lp, int64_t ldl, double* tile_inv,
                               int64_t M, int* info_dev, hipStream_t st, const char* who) {
    const int64_t dp = k.dp, Np = k.Np, cp = k.cp;
    double* Yk = Yp + M * ldy;
    double* Lkp = Lp + M * ldl;
    hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)N), dim3(256), 0, st, k.Yt, dp, Yk, ldy, (int)N, (int)dp, 1.0);
    if (M > 0) {
        // B = Yk Yp^T: few output tiles, dp deep — the contraction is split, the partials added into zeros
        hipLaunchKernelGGL(zero2d_f64_kernel, dim3((unsigned)N, 1u), dim3(256), 0, st, k.B, cp, (int64_t)0, (int)M);
        {
            ScopedProf sp(KC_ASSEMBLE, st);
            GemmShape g{Yk, ldy, Yp, ldy, (int)N, (int)M, (int)dp, 0};
            launch_gemm_f64<true, true>(g, EpiAxpby{k.B, cp, 1.0, 1.0}, st);
        }
        trsm_forward(Lp, ldl, M, NB, tile_inv, k.B, cp, Lkp, ldl, (int)N, st);      // Lkp = B Lp^-T
    }
    assemble_schur_system(Yk, ldy, dp, Lkp, ldl, M, k.S, (int)N, (int)Np, st);
    const XrowJob xj{k.XT, Np, k.TT};
    EMCID_TRY(cholesky_impl(k.S, k.LS, Np, Np, k.invS, info_dev, st, nullptr, cholesky_takes_shadow(Np) ? &xj : nullptr));
    hipLaunchKernelGGL(append_factor_kernel, dim3((unsigned)N), dim3(256), 0, st, k.LS, Np, Lp, ldl, (int)M, (int)N);
    {
        ScopedProf sp(KC_INV_BLOCK, st);
        const unsigned tiles = (unsigned)((M + N - 1) / NB - M / NB + 1);
        hipLaunchKernelGGL(tile_inverse_extend_kernel, dim3(tiles, NB / 16), dim3(64), 0, st, Lp, ldl, tile_inv, (int)M, (int)(M + N));
    }
    return check_launch(who);
}

}  // namespace emcid

using namespace emcid;

extern "C" {

/* ---- fold a preserved key set into the base factor (edit sessions) -------------------------------------------------------------
 * A session whose preserved set is full takes its M rows into a factor of its own: with P the stacked (scaled) keys,
 *     A' = A0 + P^T P,   P = Yp L_s^T,   L_s = sqrt(lam_ratio) L_src   (Yp = P L_s^-T is what the steps kept),
 * and A' is factored like lam C' itself, so every dual stage runs on it unchanged with M = 0.  `base` carries A0 (and every
 * earlier fold's P^T P) in fp64 between folds: the SYRK accumulates into it, the factorization consumes a copy.
 * Both kernels walk the NB x NB tiles on and below the block diagonal, one tile per workgroup, 128 bits per access. */
__device__ __forceinline__ void lower_tile_of(int t, int& I, int& J) {      // t = I (I + 1) / 2 + J, J <= I
    I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    J = t - I * (I + 1) / 2;
}

// base = lam * double(fl32(fl32(C * cw) / 0.5f)) inside [0, d)^2, identity on the padding: scale_cov_kernel's values for one layer
// (the diagonal tiles are filled whole: the SYRK that follows reads and writes whole tiles)
__global__ __launch_bounds__(256) void fold_base_fill_kernel(const float* __restrict__ C, int d, int dp, double lam, float cw,
                                                             double* __restrict__ base) {
    int I, J;
    lower_tile_of((int)blockIdx.x, I, J);
    for (int e = threadIdx.x; e < NB * (NB / 2); e += 256) {
        const int i = I * NB + e / (NB / 2), j = J * NB + 2 * (e % (NB / 2));
        double2 v;
        if (i < d) {
            const float* row = C + (int64_t)i * d;
            const float c0 = j < d ? row[j] * cw : 0.0f, c1 = j + 1 < d ? row[j + 1] * cw : 0.0f;
            v.x = j < d ? lam * (double)(c0 / 0.5f) : 0.0;
            v.y = j + 1 < d ? lam * (double)(c1 / 0.5f) : 0.0;
        } else {
            v.x = i == j ? 1.0 : 0.0;
            v.y = i == j + 1 ? 1.0 : 0.0;
        }
        *reinterpret_cast<double2*>(base + (int64_t)i * dp + j) = v;
    }
}

// dst = gain * src on the same tiles; lower_only: zeros above the diagonal inside the diagonal tiles (a factor as the
// factorization leaves it holds no defined values there, and a triangular GEMM hint skips K tiles, not elements)
__global__ __launch_bounds__(256) void fold_copy_lower_kernel(const double* __restrict__ src, double* __restrict__ dst, int dp,
                                                              double gain, int lower_only) {
    int I, J;
    lower_tile_of((int)blockIdx.x, I, J);
    for (int e = threadIdx.x; e < NB * (NB / 2); e += 256) {
        const int i = I * NB + e / (NB / 2), j = J * NB + 2 * (e % (NB / 2));
        const int64_t at = (int64_t)i * dp + j;
        double2 v = *reinterpret_cast<const double2*>(src + at);
        v.x = (lower_only && j > i) ? 0.0 : v.x * gain;
        v.y = (lower_only && j + 1 > i) ? 0.0 : v.y * gain;
        *reinterpret_cast<double2*>(dst + at) = v;
    }
}

// base -= sum_r a_r a_r^T over the released rows a_r = archive[rel_idx[r]] on one NB x NB tile of the block lower triangle, and
// the tile written twice: to base and to the M region the factorization consumes (the fold's third copy launch, fused).  256
// threads as 16 x 16, a thread holds rows 8 ty .. 8 ty + 7 and the double2 columns 2 tx + 32 c (c < 4) in registers; the two
// 128-wide segments of DD_ROWS released rows at a time go through LDS (2 x DD_ROWS x 1 KiB = 32 KiB; at ~236 VGPRs two
// workgroups share a compute unit, 64 of its 160 KiB, and one loads while the other multiplies; the a_i reads are one address
// per 16 lanes, the a_j reads 16 bytes per lane in lane order).  An index outside [0, n_rows), and the tail of the last chunk,
// enter as zeros.  n_rel = 0: the copy alone.
constexpr int DD_ROWS = 16;
__global__ __launch_bounds__(256) void fold_downdate_kernel(const double* __restrict__ archive, int64_t lda,
                                                            const int32_t* __restrict__ rel_idx, int n_rel, int n_rows,
                                                            double* __restrict__ base, double* __restrict__ Mb, int dp) {
    int I, J;
    lower_tile_of((int)blockIdx.x, I, J);
    __shared__ __align__(16) double S[2][DD_ROWS][NB];      // [0]: the tile's row segment of a released row, [1]: its column segment
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double2 acc[8][4];
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 4; ++c)
            acc[r][c] = *reinterpret_cast<const double2*>(base + (int64_t)(I * NB + 8 * ty + r) * dp + J * NB + 2 * tx + 32 * c);
    for (int k0 = 0; k0 < n_rel; k0 += DD_ROWS) {
        __syncthreads();      // (the chunk before has been consumed)
        for (int e = threadIdx.x; e < DD_ROWS * NB; e += 256) {        // DD_ROWS x (64 + 64) double2
            const int rr = e / NB, seg = (e % NB) / (NB / 2), c2 = e % (NB / 2);
            const int k = k0 + rr;
            const int row = k < n_rel ? rel_idx[k] : -1;
            double2 v = make_double2(0.0, 0.0);
            if (row >= 0 && row < n_rows)
                v = *reinterpret_cast<const double2*>(archive + (int64_t)row * lda + (seg ? J : I) * NB + 2 * c2);
            *reinterpret_cast<double2*>(&S[seg][rr][2 * c2]) = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int rr = 0; rr < DD_ROWS; ++rr) {
            double a[8];
            double2 b[4];
            for (int q = 0; q < 4; ++q) {
                const double2 t = *reinterpret_cast<const double2*>(&S[0][rr][8 * ty + 2 * q]);
                a[2 * q] = t.x;
                a[2 * q + 1] = t.y;
            }
            for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const double2*>(&S[1][rr][2 * tx + 32 * c]);
            for (int r = 0; r < 8; ++r)
                for (int c = 0; c < 4; ++c) {
                    acc[r][c].x -= a[r] * b[c].x;
                    acc[r][c].y -= a[r] * b[c].y;
                }
        }
    }
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 4; ++c) {
            const int64_t at = (int64_t)(I * NB + 8 * ty + r) * dp + J * NB + 2 * tx + 32 * c;
            *reinterpret_cast<double2*>(base + at) = acc[r][c];
            *reinterpret_cast<double2*>(Mb + at) = acc[r][c];
        }
}

// The first two stages of a fold, for one layer: the M preserved keys back from factor coordinates, Q [M][ldq] = Yp L_s^T against
// a clean lower-triangular copy of L_s = gain Lsrc in the M region Mb, then base += Q^T Q on the lower tiles (C != null: base
// filled from the statistics first).  Q stays where it is written: a fold's scratch, or the tail of a session's archive.
static void fold_rows_into_base(const double* Lsrc, double gain, const double* Yp, int64_t ldy, int64_t M, int64_t dp, double* Mb,
                                double* Q, int64_t ldq, double* base, const float* C, int64_t d, double lam, float cw,
                                hipStream_t st) {
    const int64_t nt = dp / NB;
    const unsigned n_tri = (unsigned)(nt * (nt + 1) / 2);
    hipLaunchKernelGGL(fold_copy_lower_kernel, dim3(n_tri), dim3(256), 0, st, Lsrc, Mb, (int)dp, gain, 1);
    {
        ScopedProf sp(KC_INV_APPLY, st);
        GemmShape g{Yp, ldy, Mb, dp, (int)M, (int)dp, (int)dp, 0};
        g.tri = 1;       // B(k, n) = L_s[n][k], zero for k > n
        g.pair = 1;
        launch_gemm_f64<true, true>(g, EpiAxpby{Q, ldq, 1.0, 0.0}, st, 2);
    }
    if (C) hipLaunchKernelGGL(fold_base_fill_kernel, dim3(n_tri), dim3(256), 0, st, C, (int)d, (int)dp, lam, cw, base);
    {
        ScopedProf sp(KC_ASSEMBLE, st);      // base += Q^T Q on the lower tiles: both operands stored [K = M][dp]
        GemmShape g{Q, ldq, Q, ldq, (int)dp, (int)dp, (int)M, 1};
        launch_gemm_f64<false, false>(g, EpiAxpby{base, dp, 1.0, 1.0}, st);
    }
}

int64_t emcid_cov_factor_fold_workspace_bytes(int64_t M, int64_t d) {
    if (M <= 0 || d <= 0) return 0;
    return M * round_up(d, NB) * (int64_t)sizeof(double);          // Q = Yp L_s^T [M, dp]
}

int emcid_cov_factor_fold_f64(const void* src_ws, double lam_ratio, const double* Yp, int64_t ldy, int64_t M, int64_t capacity,
                              const float* C, double lam, double edit_weight, int fill_base, void* dst_ws, int64_t n_layers,
                              int64_t d, int64_t layer_index, double* base, void* workspace, int64_t workspace_bytes,
                              int* info_dev, void* stream) {
    EMCID_CHECK_ARG(src_ws && dst_ws && Yp && base && workspace && info_dev && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers);
    EMCID_CHECK_ARG(M > 0 && M <= capacity && capacity < (int64_t)1 << 30);
    EMCID_CHECK_ARG(lam_ratio > 0.0 && lam_ratio < 1e300);
    EMCID_CHECK_ARG(src_ws != dst_ws || lam_ratio == 1.0);      // in place: the caller's own workspace, at the caller's own lam
    EMCID_CHECK_ARG(!fill_base || (C && lam > 0.0 && lam < 1e300 && edit_weight >= 0.0 && edit_weight <= 1.0));
    const CovFactorLayout cov(n_layers, d);
    const int64_t dp = cov.dp, nt = dp / NB;
    EMCID_CHECK_ARG(aligned16(src_ws) && aligned16(dst_ws) && aligned16(Yp) && aligned16(base) && aligned16(workspace));
    EMCID_CHECK_ARG(ldy >= dp && ldy % 2 == 0);
    EMCID_CHECK_WORKSPACE(workspace_bytes, emcid_cov_factor_fold_workspace_bytes(M, d), " (see emcid_cov_factor_fold_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    double* Mb = cov.M(dst_ws, layer_index);                 // consumed by the factorization; scratch before and after
    double *Lb = cov.L(dst_ws, layer_index), *Ib = cov.I(dst_ws, layer_index), *Xb = cov.X(dst_ws, layer_index);
    fold_rows_into_base(cov.L(src_ws, layer_index), sqrt(lam_ratio), Yp, ldy, M, dp, Mb, (double*)workspace, dp, base,
                        fill_base ? C : nullptr, d, lam, (float)(1.0 - edit_weight), st);
    hipLaunchKernelGGL(fold_copy_lower_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, base, Mb, (int)dp, 1.0, 0);
    EMCID_TRY(cholesky_serial(Mb, Lb, dp, dp, Ib, info_dev, st, 1, cov.s_mat, cov.s_inv));
    EMCID_TRY(build_full_inverse(Lb, dp, dp, Ib, Xb, Mb, cov.s_mat, 1, cov.s_mat, cov.s_inv, st));
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- release across a fold (edit sessions that keep the rows their folds added) ------------------------------------------------
 * A fold adds q_i q_i^T for the rows Q = Yp L_s^T it leaves in its scratch; a session that keeps those rows (its ARCHIVE, [rows][lda]
 * fp64) releases folded ones without a Cholesky downdate: subtract the same q_i q_i^T from base and factor base again.  The
 * update entry does, for ONE layer, in place on the session's own workspace at lam_ratio 1: the M live rows into the archive's
 * tail as Q (a fold's first two stages), then base -= the released rows, archived and just-added alike, through one index list,
 * the result copied to the layer's M region.  The refactor entry then factors the M regions of ALL layers as one batched chain. */
int emcid_session_refold_update_f64(void* cov_ws, int64_t n_layers, int64_t d, int64_t layer_index, const double* Yp, int64_t ldy,
                                    int64_t M, int64_t capacity, double* archive, int64_t lda, int64_t n_archived,
                                    const int32_t* rel_idx_dev, int64_t n_rel, double* base, void* stream) {
    EMCID_CHECK_ARG(cov_ws && archive && base && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers);
    EMCID_CHECK_ARG(M >= 0 && M <= capacity && capacity < (int64_t)1 << 30 && n_rel >= 0 && M + n_rel > 0);
    EMCID_CHECK_ARG(n_archived >= 0 && n_archived + M < (int64_t)1 << 31 && n_rel < (int64_t)1 << 31);
    EMCID_CHECK_ARG((M == 0 || Yp) && (n_rel == 0 || rel_idx_dev));
    const CovFactorLayout cov(n_layers, d);
    const int64_t dp = cov.dp, nt = dp / NB;
    EMCID_CHECK_ARG(aligned16(cov_ws) && aligned16(Yp) && aligned16(archive) && aligned16(base));
    EMCID_CHECK_ARG(lda >= dp && lda % 2 == 0 && (M == 0 || (ldy >= dp && ldy % 2 == 0)));
    hipStream_t st = (hipStream_t)stream;
    double* Mb = cov.M(cov_ws, layer_index);
    if (M > 0)
        fold_rows_into_base(cov.L(cov_ws, layer_index), 1.0, Yp, ldy, M, dp, Mb, archive + n_archived * lda, lda, base, nullptr, d,
                            0.0, 0.0f, st);
    {
        ScopedProf sp(KC_ASSEMBLE, st);
        hipLaunchKernelGGL(fold_downdate_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, archive, lda, rel_idx_dev,
                           (int)n_rel, (int)(n_archived + M), base, Mb, (int)dp);
    }
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_cov_factor_refactor_f64(void* cov_ws, int64_t workspace_bytes, int64_t n_layers, int64_t d, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(cov_ws && info_dev && n_layers > 0 && n_layers <= 32 && d > 0 && d <= 32768 && aligned16(cov_ws));
    const CovFactorLayout cov(n_layers, d);
    EMCID_CHECK_WORKSPACE(workspace_bytes, cov.total * (int64_t)sizeof(double), " (see emcid_cov_factor_workspace_bytes)");
    // every layer at once, as emcid_factor_cov_f64 runs them; eagerly: the chain is the session's, once per release
    EMCID_TRY(cholesky_serial(cov.M(cov_ws, 0), cov.L(cov_ws, 0), cov.dp, cov.dp, cov.I(cov_ws, 0), info_dev, (hipStream_t)stream,
                              (int)n_layers, cov.s_mat, cov.s_inv));
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- dual solver, apply-only form, with a PRESERVED key set (edit sessions) ------------------------------------------------
 * The keys of earlier steps enter the preserved second moment: A = lam C' + P^T P + Kt^T Kt, P the stacked earlier Kt.  In factor
 * coordinates (Yp = P X^T, rows kept verbatim, Lp = chol(I + Yp Yp^T)) a step with N new rows is a bordered Cholesky:
 *     B = Yk Yp^T,  Lkp = B Lp^-T,  T = I + Yk Yk^T - Lkp Lkp^T = Lkk Lkk^T,  Zk = T^-1 Rt,  Zp = -Lp^-T (Lkp^T Zk),
 *     U = (Zk^T Yk + Zp^T Yp) X,  W = W0 + float(U)
 * and the rows Yk, [Lkp Lkk] (and the inverses of the diagonal tiles they touch) are written behind row M of the caller's state. */
int64_t emcid_edit_dual_preserve_workspace_bytes(int64_t N, int64_t d, int64_t h, int64_t capacity) {
    if (N <= 0 || d <= 0 || h <= 0 || capacity < N) return 0;
    return PreserveWorkspace(N, d, h, capacity).total * (int64_t)sizeof(double);
}

int emcid_edit_layer_dual_preserve_f64(const float* K, const float* Zc, const float* zs_t, int64_t N, int64_t d, int64_t h,
                                       double edit_weight, int layers_left, double lam_ratio, const void* cov_factor_ws,
                                       int64_t n_layers, int64_t layer_index, double* Yp, int64_t ldy, double* Lp, int64_t ldl,
                                       double* tile_inv, int64_t capacity, int64_t M, const float* W0, float* W, float* dW_out,
                                       double* U_out, void* workspace, int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(N > 0 && d > 0 && h > 0 && Yp && Lp && tile_inv && workspace && info_dev && cov_factor_ws);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers && (W || dW_out || U_out) && ((W == nullptr) || (W0 != nullptr)));
    EMCID_CHECK_ARG(session_state_ok(M, N, d, Yp, ldy, Lp, ldl, tile_inv, capacity));
    PreserveWorkspace pw(N, d, h, capacity);
    const DualWorkspace& ws = pw.dual;
    EMCID_CHECK_WORKSPACE(workspace_bytes, pw.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    // Kt64, Rt and Yt = Kt64 X^T, exactly as the plain apply-only form
    EMCID_TRY(emcid_edit_dual_apply_stage1_f64(K, Zc, zs_t, N, d, h, edit_weight, layers_left, lam_ratio, cov_factor_ws, n_layers,
                                               layer_index, 0, N, 1, workspace, ws.total * (int64_t)sizeof(double), stream));
    double* base = (double*)workspace;
    const KeyHalf k = pw.key_half(base);
    double *R = base + ws.off_R, *RT = base + ws.off_PT, *Y2 = base + ws.off_Y2, *V = base + ws.off_V, *U = base + ws.off_U;
    double *ZT = base + pw.off_ZT, *G = base + pw.off_G;
    const int64_t dp = ws.dp, Np = ws.Np, cp = pw.cp;
    double* Lkp = Lp + M * ldl;
    EMCID_TRY(session_append_rows(k, N, Yp, ldy, Lp, ldl, tile_inv, M, info_dev, st, __func__));
    // RT[h, Np] = Rt^T ; Zk^T = RT T^-1
    EMCID_TRY(solve_schur_rhs(R, ws.hp, h, Np, k.LS, k.invS, cholesky_takes_shadow(Np) ? k.XT : nullptr, k.S, RT, Y2, ws.y2_doubles(), st));
    // ZT = [Zp^T | Zk^T] [h, M + N]: then V = ZT [Yp; Yk] is ONE product over the state's rows, the new ones included
    hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)h), dim3(256), 0, st, RT, Np, ZT + M, cp, (int)h, (int)N, 1.0);
    if (M > 0) {
        {
            ScopedProf sp(KC_DELTA_W, st);       // G[h, M] = -(Zk^T Lkp)
            GemmShape g{RT, Np, Lkp, ldl, (int)h, (int)M, (int)N, 0};
            launch_gemm_f64<true, false>(g, EpiAxpby{G, cp, -1.0, 0.0}, st);
        }
        trsm_backward(Lp, ldl, M, NB, tile_inv, G, cp, ZT, cp, (int)h, st);      // Zp^T = G Lp^-1
    }
    {
        ScopedProf sp(KC_DELTA_W, st);           // V[h, dp] = Zp^T Yp + Zk^T Yk
        GemmShape g{ZT, cp, Yp, ldy, (int)h, (int)dp, (int)(M + N), 0};
        launch_gemm_f64<true, false>(g, EpiAxpby{V, dp, 1.0, 0.0}, st);
    }
    apply_inverse_backward(CovFactorLayout(n_layers, d).X(cov_factor_ws, layer_index), dp, V, (int)h, (int)dp, U, dp, st, base + ws.off_SK);
    if (W || dW_out) hipLaunchKernelGGL(apply_u2d_kernel, dim3((unsigned)h), dim3(256), 0, st, U, dp, W0, W, dW_out, (int)d);
    if (U_out) hipLaunchKernelGGL(copy2d_f64_kernel, dim3((unsigned)h), dim3(256), 0, st, U, dp, U_out, d, (int)h, (int)d, 1.0);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* ---- edit sessions: a RETAIN list — preserved rows with a zero residual -------------------------------------------------------
 * The first half of emcid_edit_layer_dual_preserve_f64 for keys that are to stay where they are: Yk, B, Lkp, T, its Cholesky and
 * the append behind row M.  With Rt = 0 the step's Zk, Zp and U vanish identically, so that half is not run at all: no Zc, no
 * targets, no weights. */
int64_t emcid_session_retain_workspace_bytes(int64_t N, int64_t d, int64_t capacity) {
    if (N <= 0 || d <= 0 || capacity < N) return 0;
    return RetainWorkspace(N, d, capacity).total * (int64_t)sizeof(double);
}

int emcid_session_retain_f64(const float* K, int64_t N, int64_t d, double row_scale, double lam_ratio, const void* cov_factor_ws,
                             int64_t n_layers, int64_t layer_index, double* Yp, int64_t ldy, double* Lp, int64_t ldl,
                             double* tile_inv, int64_t capacity, int64_t M, void* workspace, int64_t workspace_bytes, int* info_dev,
                             void* stream) {
    EMCID_CHECK_ARG(K && N > 0 && d > 0 && Yp && Lp && tile_inv && workspace && info_dev && cov_factor_ws);
    EMCID_CHECK_ARG(0 <= layer_index && layer_index < n_layers && row_scale > 0.0 && row_scale < 1e150);
    EMCID_CHECK_ARG(lam_ratio > 0.0 && lam_ratio < 1e300);
    EMCID_CHECK_ARG(session_state_ok(M, N, d, Yp, ldy, Lp, ldl, tile_inv, capacity));
    RetainWorkspace ws(N, d, capacity);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    double *Kt = base + ws.off_K, *Yt = base + ws.off_Y;
    const int64_t dp = ws.dp, Np = ws.Np;
    {
        ScopedProf sp(KC_PREP, st);
        hipLaunchKernelGGL(prep_k_kernel, dim3((unsigned)Np), dim3(256), 0, st, K, (int)N, (int)d, row_scale, Kt, (int)dp,
                           1.0 / sqrt(lam_ratio));
    }
    // Yt = Kt64 X^T over the Np padded rows, as stage 1 of the apply-only form runs the whole concept range
    apply_inverse_forward(CovFactorLayout(n_layers, d).X(cov_factor_ws, layer_index), dp, Kt, Yt, (int)Np, st, base + ws.off_SK);
    return session_append_rows(ws.key_half(base), N, Yp, ldy, Lp, ldl, tile_inv, M, info_dev, st, __func__);
}

/* ---- edit sessions: RELEASE rows of the preserved set ----------------------------------------------------------------------------
 * keep[0 .. n_keep) are the rows that stay, ascending, keep[j] == j below `first` (the smallest released index).  Rows < first of
 * Yp, Lp and the tile inverses already are the state of the reduced set (the leading rows of a Cholesky factor do not depend on
 * later ones).  The kept rows behind `first` are gathered into the workspace's Yt block — source and destination rows overlap in
 * Yp — and re-enter as the key half of a step with M = first, N = n_keep - first: no forward, no X, no statistics, no weights. */
int64_t emcid_session_release_workspace_bytes(int64_t n_rebuilt, int64_t d, int64_t capacity) {
    return emcid_session_retain_workspace_bytes(n_rebuilt, d, capacity);
}

int emcid_session_release_f64(const int32_t* keep_dev, int64_t n_keep, int64_t first, int64_t d, double* Yp, int64_t ldy, double* Lp,
                              int64_t ldl, double* tile_inv, int64_t capacity, int64_t M, void* workspace, int64_t workspace_bytes,
                              int* info_dev, void* stream) {
    EMCID_CHECK_ARG(keep_dev && d > 0 && Yp && Lp && tile_inv && workspace && aligned16(workspace) && info_dev);
    EMCID_CHECK_ARG(first < n_keep && n_keep < M && M <= capacity);
    const int64_t N = n_keep - first;
    EMCID_CHECK_ARG(session_state_ok(first, N, d, Yp, ldy, Lp, ldl, tile_inv, capacity));
    RetainWorkspace ws(N, d, capacity);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    hipLaunchKernelGGL(gather_rows_f64_kernel, dim3((unsigned)ws.Np), dim3(256), 0, st, Yp, ldy, keep_dev + first, (int)N, (int)M,
                       base + ws.off_Y, (int)ws.dp);
    return session_append_rows(ws.key_half(base), N, Yp, ldy, Lp, ldl, tile_inv, first, info_dev, st, __func__);
}

/* ---- edit sessions: RESCALE rows of the preserved set ----------------------------------------------------------------------------
 * Row i of the state becomes factors[i] * row i of src_Yp for first <= i < M (src_Yp may be Yp itself, or a copy of it: a sweep
 * scales out of a backup into the live state); factors[i] == 1 below `first` is the caller's word and nothing below it is read or
 * written.  A new (lam, edit_weight) multiplies every row by sqrt(a / a'), a = 2 lam (1 - e): chol(a' C) = sqrt(a' / a) chol(a C);
 * a new weight of a concept multiplies its rows by sqrt(w' / w).  Lp and the tile inverses behind `first` are stale either way:
 * the scaled rows go through the workspace's Yt block and re-enter as the key half of a step with M = first, N = M - first, as a
 * release's kept rows do — no forward, no X, no statistics, no weights. */
int emcid_session_rescale_f64(const double* factors_dev, const double* src_Yp, int64_t lds, int64_t first, int64_t d, double* Yp,
                              int64_t ldy, double* Lp, int64_t ldl, double* tile_inv, int64_t capacity, int64_t M, void* workspace,
                              int64_t workspace_bytes, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(factors_dev && src_Yp && d > 0 && Yp && Lp && tile_inv && workspace && aligned16(workspace) && info_dev);
    EMCID_CHECK_ARG(0 <= first && first < M && M <= capacity);
    const int64_t N = M - first;
    EMCID_CHECK_ARG(session_state_ok(first, N, d, Yp, ldy, Lp, ldl, tile_inv, capacity));
    EMCID_CHECK_ARG(aligned16(src_Yp) && lds >= round_up(d, NB) && lds % 2 == 0);
    RetainWorkspace ws(N, d, capacity);
    EMCID_CHECK_WORKSPACE(workspace_bytes, ws.total * (int64_t)sizeof(double), "");
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)workspace;
    hipLaunchKernelGGL(scale_rows_f64_kernel, dim3((unsigned)ws.Np), dim3(256), 0, st, src_Yp, lds, factors_dev, (int)first, (int)N,
                       base + ws.off_Y, (int)ws.dp);
    return session_append_rows(ws.key_half(base), N, Yp, ldy, Lp, ldl, tile_inv, first, info_dev, st, __func__);
}

/* The readout of the preserve step that has just run on `workspace` (same N, d, h, capacity, M, same stream): the step left
 * ZT = [Zp^T | Zk^T] [h][M + N] and Rt [N][h] there.  One launch. */
int emcid_session_step_norms_f64(const void* workspace, int64_t workspace_bytes, int64_t N, int64_t d, int64_t h, int64_t capacity,
                                 int64_t M, double* drift_out, double* left_out, double* resid_out, void* stream) {
    EMCID_CHECK_ARG(workspace && N > 0 && d > 0 && h > 0 && left_out && resid_out && (drift_out || M == 0));
    EMCID_CHECK_ARG(M >= 0 && M + N <= capacity && capacity < (int64_t)1 << 30);
    PreserveWorkspace pw(N, d, h, capacity);
    EMCID_CHECK_WORKSPACE(workspace_bytes, pw.total * (int64_t)sizeof(double), "");
    const double* base = (const double*)workspace;
    const double *R = base + pw.dual.off_R, *ZT = base + pw.off_ZT;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(step_norms_kernel, dim3((unsigned)((M + 2 * N + 3) / 4)), dim3(256), 0, st, ZT, pw.cp, R, pw.dual.hp, (int)h,
                       (int)M, (int)N, drift_out, left_out, resid_out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

}  // extern "C"
