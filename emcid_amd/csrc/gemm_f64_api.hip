// The fp64 GEMM family of gemm_f64.h behind the C ABI: plain, with structure hints and K splits, batched, and two-phase stream-K
// (tests and scripts drive the tile forms directly through these; the solvers call the launchers themselves).  The kernels are
// spd_solve.hip's instantiations.
#include "spd_solve.h"

using namespace emcid;

// ta / tb == 0: K contiguous ([rows][K]); 1: rows contiguous ([K][rows])
static void launch_by_layout(int ta, int tb, const GemmShape& p, const EpiAxpby& e, hipStream_t st, int cfg = -1) {
    if (ta == 0 && tb == 0) launch_gemm_f64<true, true>(p, e, st, cfg);
    else if (ta == 0 && tb == 1) launch_gemm_f64<true, false>(p, e, st, cfg);
    else if (ta == 1 && tb == 0) launch_gemm_f64<false, true>(p, e, st, cfg);
    else launch_gemm_f64<false, false>(p, e, st, cfg);
}

extern "C" {

int emcid_dgemm_f64(int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                    const double* B, int64_t ldb, double beta, double* C, int64_t ldc, void* stream) {
    EMCID_CHECK_ARG(M > 0 && N > 0 && K > 0 && A && B && C);
    EMCID_CHECK_ARG(aligned16(A) && aligned16(B) && (lda % 2 == 0) && (ldb % 2 == 0));
    EMCID_CHECK_ARG(M < (1 << 30) && N < (1 << 30) && K < (1 << 30));
    hipStream_t st = (hipStream_t)stream;
    GemmShape p{A, lda, B, ldb, (int)M, (int)N, (int)K, 0};
    EpiAxpby e{C, ldc, alpha, beta};
    ScopedProf sp(KC_DGEMM, st);
    launch_by_layout(ta, tb, p, e, st);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_dgemm_ex_f64(int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                       const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int flags, int cfg, int ksplit,
                       void* stream) {
    EMCID_CHECK_ARG(M > 0 && N > 0 && K > 0 && A && B && C);
    EMCID_CHECK_ARG(aligned16(A) && aligned16(B) && (lda % 2 == 0) && (ldb % 2 == 0));
    EMCID_CHECK_ARG(M < (1 << 30) && N < (1 << 30) && K < (1 << 30) && cfg >= -1 && cfg <= 2 && (flags & ~63) == 0);
    EMCID_CHECK_ARG(ksplit == 0 || beta == 1.0);
    hipStream_t st = (hipStream_t)stream;
    GemmShape p{A, lda, B, ldb, (int)M, (int)N, (int)K, (flags >> 4) & 1};
    p.tri = flags & 15;
    p.pair = (flags >> 5) & 1;
    if (ksplit > 0) p.ksplit = ksplit;
    if (ksplit < 0) p.kchunk = -ksplit;
    EpiAxpby e{C, ldc, alpha, beta};
    ScopedProf sp(KC_DGEMM, st);
    launch_by_layout(ta, tb, p, e, st, cfg);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int64_t emcid_streamk_workspace_bytes(int wgs) { return wgs > 0 ? streamk_workspace_doubles(wgs) * (int64_t)sizeof(double) : 0; }

int emcid_dgemm_streamk_f64(int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, const double* B,
                            int64_t ldb, double* C, int64_t ldc, int flags, int wgs, double diag_add, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    EMCID_CHECK_ARG(M > 0 && N > 0 && K > 0 && A && B && C && workspace && wgs > 0 && wgs <= 4096);
    EMCID_CHECK_ARG(aligned16(A) && aligned16(B) && aligned16(workspace) && (lda % 2 == 0) && (ldb % 2 == 0));
    EMCID_CHECK_ARG(M < (1 << 30) && N < (1 << 30) && K < (1 << 30) && (flags & ~19) == 0);
    const int tri = flags & 3, lower = (flags >> 4) & 1;
    EMCID_CHECK_ARG((lower && M == N && tri == 0) || (!lower && (tri == 1 || tri == 2)));
    EMCID_CHECK_ARG(((M + 127) / 128) * ((N + 127) / 128) <= 16384);      // one ticket counter per 128 x 128 tile
    EMCID_CHECK_WORKSPACE(workspace_bytes, emcid_streamk_workspace_bytes(wgs), "");
    hipStream_t st = (hipStream_t)stream;
    GemmShape p{A, lda, B, ldb, (int)M, (int)N, (int)K, lower};
    p.tri = tri;
    ScopedProf sp(KC_DGEMM, st);
    const bool launched = tb == 0 ? launch_gemm_f64_streamk2<true, true>(p, EpiAxpby{C, ldc, alpha, 0.0}, st, wgs, (double*)workspace, diag_add)
                                  : launch_gemm_f64_streamk2<true, false>(p, EpiAxpby{C, ldc, alpha, 0.0}, st, wgs, (double*)workspace, diag_add);
    if (!launched) return fail(EMCID_ERR_BAD_ARG, __func__, "more 128 x 128 output tiles than ticket counters (16384)");
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

/* diagnostic: later two-phase stream-K launches write 8 shader-clock values per workgroup to stamps_dev (NULL: stop) —
 * [0] start, [1] end, cycles in [2] K loops, [3] partial-tile publishes, [4] last-ticket reductions, [5] epilogues,
 * [6] segments, [7] run index */
int emcid_debug_streamk_stamps(long long* stamps_dev) {
    g_streamk_stamps = stamps_dev;
    return EMCID_OK;
}

int emcid_dgemm_batched_f64(int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                            int64_t sA, const double* B, int64_t ldb, int64_t sB, double beta, double* C, int64_t ldc, int64_t sC,
                            int64_t batch, void* stream) {
    EMCID_CHECK_ARG(M > 0 && N > 0 && K > 0 && A && B && C && batch > 0 && batch <= 65535);
    EMCID_CHECK_ARG(aligned16(A) && aligned16(B) && (lda % 2 == 0) && (ldb % 2 == 0) && (sA % 2 == 0) && (sB % 2 == 0));
    EMCID_CHECK_ARG(M < (1 << 30) && N < (1 << 30) && K < (1 << 30) && sA >= 0 && sB >= 0 && sC >= 0);
    hipStream_t st = (hipStream_t)stream;
    GemmShape p{A, lda, B, ldb, (int)M, (int)N, (int)K, 0};
    p.sA = sA; p.sB = sB; p.batch = (int)batch;
    EpiAxpby e{C, ldc, alpha, beta};
    e.sC = sC;
    ScopedProf sp(KC_DGEMM, st);
    // no K split is asked for here; the launcher's own rule still applies: with beta == 1, small tiles, fewer than 512
    // workgroups over the whole batch and K >= 256 it splits K (blockIdx.z = batch * ksplit + split) and adds the partials
    // with f64 atomics.  The per-edit Grams of the UCE closed form call this with beta == 0 and are never split.
    launch_by_layout(ta, tb, p, e, st);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

}  // extern "C"
