// What the units of the fp64 solver library share (internal, not installed): the factorization, solves and inverse builders of
// spd_solve.hip, the workspace layouts more than one unit addresses, and the element-wise kernels more than one unit launches.
//   runtime.hip       last error, per-class event profiler, ABI version, env_flag, the hipGraph cache (interface: common.h)
//   spd_solve.hip     Cholesky device code and schedules, block inverses, triangular solves, explicit inverse and its products;
//                     the one place the fp64 GEMM kernels are instantiated
//   gemm_f64_api.hip  the C entries of the fp64 GEMM family
//   edit_solve.hip    primal solver, covariance-factor workspace, the dual / apply-only / column-sharded forms
//   session.hip       edit sessions: preserve, retain, release, step norms, fold, release across a fold
#pragma once
#include "common.h"
#include "gemm_f64.h"

namespace emcid {

// ---- spd_solve.hip ------------------------------------------------------------------------------------------------------------

// The GEMM launchers these units call are instantiated in spd_solve.hip only: every kernel is in the library once, next to the
// Cholesky kernels that inline the same tiles, and a unit that only calls them compiles in seconds.  (A launcher not listed here
// still works: it is instantiated where it is called.)
#define EMCID_GEMM_F64_INSTANCES(X)                                                                        \
    X void launch_gemm_f64<true, false, EpiAxpby>(GemmShape, EpiAxpby, hipStream_t, int);                     \
    X void launch_gemm_f64<true, true, EpiAxpby>(GemmShape, EpiAxpby, hipStream_t, int);                      \
    X bool launch_gemm_f64_streamk2<true, true>(GemmShape, EpiAxpby, hipStream_t, int, double*, double);      \
    X bool launch_gemm_f64_streamk2<true, false>(GemmShape, EpiAxpby, hipStream_t, int, double*, double);     \
    X void launch_gemm_f64<false, true, EpiAxpby>(GemmShape, EpiAxpby, hipStream_t, int);                     \
    X void launch_gemm_f64<false, false, EpiAxpby>(GemmShape, EpiAxpby, hipStream_t, int);                    \
    X void launch_gemm_f64<false, false, EpiAssemble>(GemmShape, EpiAssemble, hipStream_t, int);              \
    X void launch_gemm_f64<false, false, EpiDeltaW>(GemmShape, EpiDeltaW, hipStream_t, int);                  \
    X void launch_gemm_f64<false, true, EpiDeltaW>(GemmShape, EpiDeltaW, hipStream_t, int);                   \
    X void launch_gemm_f64<true, false, EpiDeltaW>(GemmShape, EpiDeltaW, hipStream_t, int);
EMCID_GEMM_F64_INSTANCES(extern template)

// A product that does NOT depend on the matrix being factored, cut into `nslices` K slices, one per leaf launch: the leaf
// occupies ONE compute unit for ~36 us while the rest of the chip has (almost) nothing to do, so an independent GEMM of the
// caller's rides along in the launches' other workgroups ("shadow").  Used by the dual solver for P = Yt X (X = inv(L) of
// lam*C', lower triangular, stored [k][n]), which turns U = (Z^T Yt) X — a GEMM against the triangle AFTER the N x N solve, on
// the critical path — into U = Z^T P.  C = A B with B(k, n) = 0 for k < n; 64 x 128 output tiles; a workgroup takes column tile
// j and its mirror image NT-1-j (equal total depth for every workgroup) and contracts slice `slice` of each tile's own K range;
// slice 0 stores, later slices add — launches of one stream are ordered and a tile belongs to one workgroup per launch, so the
// sum order is fixed (bit-reproducible) and nothing is atomic.
struct ShadowJob {
    const double* A; int64_t lda;     // [M][K], K contiguous
    const double* B; int64_t ldb;     // [K][N], N contiguous, zero for k < n
    double* C; int64_t ldc;           // [M][N]
    int M, N, K;
    int wgs;                          // workgroups per launch: ceil(M / 64) * ceil(ceil(N / 128) / 2); 0 = no job
    long long* stamps;                // diagnostic (usually null): per launch slice and workgroup [start, mid, end, kind]
    int xcd_gx;                       // > 0: XCD-blocked tile assignment, the 8 XCDs as a xcd_gx x (8 / xcd_gx) grid (set by the launcher)
    int nofast;                       // GemmShape.nofast for the shadow tiles (EMCID_GEMM_FAST=0)
    int fuse_pair;                    // both tiles of a pair through one software pipeline (EMCID_SHADOW_FUSE, default 1)
};

// The explicit inverse of the factor, built ROW BLOCK BY ROW BLOCK inside the factorization's own launches (dual solver: XS =
// inv(LS) is what turns Z = S^-1 R into two GEMMs).  Stored transposed, Xt[n][k] = X[k][n], so that both products of a step are
// K-contiguous on both sides:
//     leaf launch j  (j >= 1):  Tt [128 j, 128] = Xt[0:128j, 0:128j] L[j, 0:j]^T        (X of the leading j blocks is complete)
//     spine launch j (j >= 0):  Xt[0:128j, j]  = -Tt inv(L_jj)^T,   Xt[j, j] = inv(L_jj)^T
// i.e. X[j, 0:j] = -inv(L_jj) L[j, 0:j] X[0:j, 0:j].  Behind the last leaf only that block row's second product is left (one
// small launch) where the recursive-halving build took six dependent ones (~70 us per layer at N = 1000).
struct XrowJob {
    double* Xt; int64_t ldx;      // [n, n] transposed inverse (every entry the consumers read is written here)
    double* Tt;                   // [n, 128] scratch, leading dimension 128
};
constexpr int SH_BM = 64, SH_BN = 128;

inline bool cholesky_takes_shadow(int64_t dp) {      // the schedule whose leaf launches can carry a ShadowJob
    return dp <= 2048 && dp >= 2 * NB;
}
int cholesky_serial(double* A, double* L, int64_t dp, int64_t lda, double* invw, int* info, hipStream_t st, int nbatch = 1,
                    int64_t s_mat = 0, int64_t s_inv = 0);
int cholesky_impl(double* A, double* L, int64_t dp, int64_t lda, double* invw, int* info, hipStream_t st,
                  const ShadowJob* shadow = nullptr, const XrowJob* xrow = nullptr);
void trsm_forward(const double* L, int64_t ldl, int64_t n, int blk, const double* inv, double* B, int64_t ldb, double* Out,
                  int64_t ldo, int rows, hipStream_t st);
void trsm_backward(const double* L, int64_t ldl, int64_t n, int blk, const double* inv, double* B, int64_t ldb, double* Out,
                   int64_t ldo, int rows, hipStream_t st);
int cholesky_solve_impl(const double* L, int64_t dp, int64_t lda, const double* invw, double* Bt, double* Yt, int64_t Mrows,
                        int64_t ldb, hipStream_t st);
// (T holds t_doubles per factor; fewer than full_inverse_scratch_doubles(dp, lda) is an error before anything is launched)
int64_t full_inverse_scratch_doubles(int64_t dp, int64_t lda);
int build_full_inverse(const double* L, int64_t dp, int64_t lda, const double* invw, double* X, double* T, int64_t t_doubles,
                       int nbatch, int64_t s_mat, int64_t s_inv, hipStream_t st);
constexpr int kStreamKWgs = 256;      // runs of the stream-K products against X (apply_inverse_*), and what their workspace is sized for
void apply_inverse_forward(const double* X, int64_t dp, const double* Kt, double* Yt, int rows, hipStream_t st,
                           double* sk_work = nullptr);
void apply_inverse_backward(const double* X, int64_t dp, const double* V, int rows, int ncols, double* C, int64_t ldc,
                            hipStream_t st, double* sk_work = nullptr);
// S[Np, Np] = I + Yk Yk^T - Lkp Lkp^T (lower tiles; rows / columns >= N stay those of the identity): the system of a session step
void assemble_schur_system(const double* Yk, int64_t ldy, int64_t dp, const double* Lkp, int64_t ldl, int64_t M, double* S, int N,
                           int Np, hipStream_t st);

// ---- workspace layouts more than one unit addresses -----------------------------------------------------------------------------

// The covariance-factor workspace (emcid_factor_cov_f64): [M | L | 512-block inverses | X = inv(L)], each region holding its
// n_layers blocks back to back.  M = lam*C' is consumed by the factorization and is scratch afterwards.  (The Python binding
// restates the offsets of L and X: include/emcid_hip.h is the contract.)
struct CovFactorLayout {
    int64_t n_layers, dp, s_mat, s_inv, total;   // doubles
    CovFactorLayout(int64_t n_layers_, int64_t d)
        : n_layers(n_layers_), dp(round_up(d, NB)), s_mat(dp * dp), s_inv(inv_doubles(dp)), total(n_layers * (3 * s_mat + s_inv)) {}
    // block of layer l (an entry that only reads its workspace takes the result as const double*)
    double* M(const void* ws, int64_t l) const { return (double*)ws + l * s_mat; }
    double* L(const void* ws, int64_t l) const { return (double*)ws + n_layers * s_mat + l * s_mat; }
    double* I(const void* ws, int64_t l) const { return (double*)ws + 2 * n_layers * s_mat + l * s_inv; }
    double* X(const void* ws, int64_t l) const { return (double*)ws + n_layers * (2 * s_mat + s_inv) + l * s_mat; }
};

struct DualWorkspace {
    int64_t Np, dp, hp;
    int64_t off_K, off_P, off_Y, off_R, off_S, off_LS, off_invS, off_PT, off_Y2, off_V, off_U, off_SK, off_XT, off_TT, total;   // doubles
    DualWorkspace(int64_t N, int64_t d, int64_t h) {
        Np = round_up(N, NB);
        dp = round_up(d, NB);
        hp = round_up(h, 2);
        int64_t o = 0;
        off_K = o; o += Np * dp;
        off_P = o; o += Np * dp;
        off_Y = o; o += Np * dp;
        off_R = o; o += Np * hp;
        off_S = o; o += Np * Np;
        off_LS = o; o += Np * Np;
        off_invS = o; o += inv_doubles(Np);
        off_PT = o; o += dp * Np;
        off_Y2 = o; o += dp * Np;
        off_V = o; o += hp * dp;
        off_U = o; o += hp * dp;
        off_SK = o; o += streamk_workspace_doubles(kStreamKWgs);      // partial-tile slots + ticket counters (zero between launches)
        off_XT = o; o += Np * Np;                                     // XrowJob: inv(LS)^T ...
        off_TT = o; o += Np * NB;                                     // ... and its per-step scratch
        total = o;
    }
    int64_t y2_doubles() const { return dp * Np; }
    // every block by name (emcid_edit_dual_block, include/emcid_hip.h: the numbers are the EMCID_DUAL_* constants there)
    bool block(int which, int64_t* off, int64_t* doubles) const {
        const int64_t offs[] = {off_K, off_P, off_Y, off_R, off_S, off_LS, off_invS, off_PT, off_Y2, off_V, off_U, off_SK, off_XT, off_TT, total};
        if (which == EMCID_DUAL_SK_COUNTERS) {      // the tail of the stream-K block: what has to be zero between launches
            *off = off_XT - 8192;
            *doubles = 8192;
            return true;
        }
        if (which < 0 || which > EMCID_DUAL_TT) return false;
        *off = offs[which];
        *doubles = offs[which + 1] - offs[which];
        return true;
    }
};

// How solve_schur_rhs forms Z^T = RT S^-1 when no inverse rode in the factorization (Np > 2048 or Np = 128).  The explicit
// inverse is built with `scratch_doubles` of Y2 as build_full_inverse's T: a dual workspace holds dp * Np there, which is too
// little for a d well below N (d = 768 keys, 2100 concepts: 1151 * 2176 + 1024 doubles asked, 768 * 2176 held), and then, as
// beyond Np = 4096, the solve is the block substitution.  The one statement of the condition: the branch and the entry points'
// form report (emcid_edit_dual_schur_form) both call it, and build_full_inverse refuses a smaller T before it launches.
inline int schur_rhs_form(int64_t Np, bool have_xt, bool have_full_inv, int64_t scratch_doubles) {
    if (have_xt) return EMCID_SCHUR_XROW;
    if (have_full_inv && Np <= 4096 && full_inverse_scratch_doubles(Np, Np) <= scratch_doubles) return EMCID_SCHUR_FULL_INVERSE;
    return EMCID_SCHUR_SUBSTITUTION;
}

// ---- edit_solve.hip -----------------------------------------------------------------------------------------------------------
int solve_schur_rhs(const double* R, int64_t hp, int64_t h, int64_t Np, const double* LS, const double* invS, const double* XT,
                    double* full_inv, double* RT, double* Y2, int64_t y2_doubles, hipStream_t st);

// ---- element-wise kernels more than one unit launches (internal linkage: every unit carries its own copy) ---------------------

static __global__ __launch_bounds__(256) void copy2d_f64_kernel(const double* __restrict__ src, int64_t lds_, double* __restrict__ dst,
                                                                 int64_t ldd, int rows, int cols, double scale = 1.0) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < cols; c += 256) dst[(int64_t)r * ldd + c] = src[(int64_t)r * lds_ + c] * scale;
}

// zero fill by kernel: a hipMemset node inside a captured graph binds the allocation object of capture time, which
// goes stale when the caller's allocator recycles the address range; a kernel only carries the raw pointer
static __global__ __launch_bounds__(256) void zero_f64_kernel(double* __restrict__ p, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) p[i] = 0.0;
}

static __global__ __launch_bounds__(256) void zero2d_f64_kernel(double* __restrict__ p, int64_t ld, int64_t s_batch, int cols) {
    double* row = p + blockIdx.y * s_batch + (int64_t)blockIdx.x * ld;
    for (int j = threadIdx.x; j < cols; j += 256) row[j] = 0.0;
}

// S = I (full square): start value of the split-K accumulation S += Yt Yt^T
static __global__ __launch_bounds__(256) void eye_f64_kernel(double* __restrict__ S, int n) {
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += 256) S[(int64_t)i * n + j] = (i == j) ? 1.0 : 0.0;
}

// W = W0 + float(U), dW = float(U) with U[h][ldu] (the apply-only dual path leaves U with the padded leading dimension)
static __global__ __launch_bounds__(256) void apply_u2d_kernel(const double* __restrict__ U, int64_t ldu, const float* __restrict__ W0,
                                                                float* __restrict__ W, float* __restrict__ dW, int d) {
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < d; j += 256) {
        const float f = (float)U[(int64_t)i * ldu + j];
        if (dW) dW[(int64_t)i * d + j] = f;
        if (W) W[(int64_t)i * d + j] = W0[(int64_t)i * d + j] + f;
    }
}

}  // namespace emcid
