// The dense SPD algebra of stage 2 on gfx950: blocked fp64 Cholesky (device code and both host schedules), the inverses of
// the diagonal blocks, the blocked triangular solves, the explicit inverse of a factor and the two products against it.
// Replaces torch.linalg.solve in fp64 of the reference (emcid/emcid_main.py:1016-1061); the solvers that call this are in
// edit_solve.hip and session.hip.
//
// Everything dense runs through gemm_f64.h (v_mfma_f64_16x16x4_f64).  The Cholesky is right-looking
// with NB = 128: a single-workgroup LDS leaf factors the diagonal block and inverts it, so the panel
// solve and every later triangular solve are MFMA GEMMs against the inverted diagonal blocks.
#include <vector>

#include "spd_solve.h"

namespace emcid {

// ---- diagonal leaf: Cholesky of one NB x NB block + its inverse, one workgroup ---------------------------
//
// The leaf is the serial spine of the factorization (d sequential pivots), so it is built for latency:
//  * the 128-block is processed as four 32-column panels;
//  * a panel's 32x32 diagonal block is factored by ONE wave entirely in registers: lane i < 32 holds row i,
//    and lanes 32..63 hold the rows of an identity appended below it.  Running the same right-looking
//    elimination on the augmented [A; I] leaves L in the top lanes and Z = L^-T in the bottom lanes
//    ([A; I] = [L; Z] L^T), so the block's inverse costs no extra instructions.  Pivot rows are broadcast
//    with v_readlane (lane index is a compile-time constant after unrolling); 1/sqrt(pivot) is v_rsq_f64
//    plus two Newton steps;
//  * the rows below the diagonal block (panel solve P = A_below * Z) and the in-leaf trailing update
//    (T -= P P^T) are f64 MFMAs straight out of the LDS image, all four waves;
//  * the inverse of the whole 128-block is assembled from the four 32x32 inverses by two levels of
//    inv([[A,0],[C,B]]) = [[A^-1,0],[-B^-1 C A^-1, B^-1]], again MFMA out of LDS.
// LDS image S[128][130]: row stride 130 doubles (= 4*65 dwords) makes the k-contiguous MFMA fragment
// reads (16 rows x 2 k) hit 64 distinct banks.

constexpr int LEAF_T = 512;   // 8 waves: wave 0 factors the diagonal sub-blocks, all 8 run the MFMA phases
constexpr int LEAF_LOAD_BATCH = 16;   // all of a thread's 16 block vectors in flight at once (8: two dependent round trips)
constexpr int SB = 32;        // register-factored diagonal sub-block
constexpr int SLD = NB + 2;   // 130
constexpr int ZLD = 48;       // temp tiles [32][48]: k-row stride == 32 (mod 64) dwords

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// one 16x16 output tile, K deep, operands fetched through address functors (doubles in LDS)
template <int K, class FA, class FB>
__device__ __forceinline__ v4d leaf_tile(const double* lds, FA fa, FB fb, int l15, int l4) {
    v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};   // two chains: dependent f64 MFMAs do not issue back to back
#pragma unroll
    for (int kk = 0; kk < K / 4; kk += 2) {
        const double a0 = lds[fa(l15, kk * 4 + l4)];
        const double b0 = lds[fb(kk * 4 + l4, l15)];
        const double a1 = lds[fa(l15, kk * 4 + 4 + l4)];
        const double b1 = lds[fb(kk * 4 + 4 + l4, l15)];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// ---- phase A on the matrix pipe ---------------------------------------------------------------------------------------
// The 32x32 diagonal block W = [T | E] (T symmetric, E = I) is held by ONE wave as 16x16 f64 MFMA accumulator tiles
// (element (row, col) of a tile sits in lane (col, row & 3), register row >> 2) and eliminated four pivot rows at a
// time:   R = inv(chol(T[p,p])) * W[p, :]   (the pivot rows become rows of [L^T | L^-1]),
//         W[i, :] -= R[:, i]^T * R           (rows below)
// In that layout a 4 x 16 slab of pivot rows is at once the MFMA B operand (k = pivot row, n = column) and — read as
// "column tile i" — the A operand of the update of row tile i (m = row, k = pivot row): no data movement between
// steps.  Scaling the slab by the inverse 4x4 factor is one more MFMA whose A operand carries that inverse in its
// first four rows; only the 4x4 factorization itself (10 values fetched with v_readlane, ~40 scalar-uniform flops)
// is outside the matrix pipe.  The lower-left T tile is never needed (its rows' pivots come later and read only
// columns right of the diagonal), so three T tiles and three E tiles are live.
struct Inv44 { double w00, w10, w11, w20, w21, w22, w30, w31, w32, w33; };

__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// 1/sqrt(p) on the pivot chain: hardware estimate + ONE third-order correction (4 dependent fp64 ops instead of the
// 6 of two Newton steps):  e = 1 - p r^2,  r <- r + r e (1/2 + 3/8 e)   (error ~ e^3)
__device__ __forceinline__ double rsqrt_chain(double p) {
    const double r = __builtin_amdgcn_rsq(p);
    const double e = fma(-p * r, r, 1.0);
    return fma(r * e, fma(e, 0.375, 0.5), r);
}

// src holds the 4x4 SPD block D at lanes 16*a + lane0 + b (a = row, b = col); returns inv(chol(D)); bad = first
// non-positive pivot (0..3) or 4.  Written for dependency depth: everything that does not need the newest
// reciprocal root is formed before it arrives.
__device__ __forceinline__ Inv44 inv_chol44(double src, int lane0, int& bad) {
    double d[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) d[a][b] = readlane_f64(src, 16 * a + lane0 + b);
    // Pivots are taken in PAIRS: for [[a, b], [b, c]] the second pivot is det/a with det = a c - b^2 (the same
    // cancellation as c - (b/sqrt a)^2), so 1/sqrt(a) and 1/sqrt(det) are refined side by side and
    // r1 = 1/sqrt(det/a) = (a r0) rsqrt(det): two reciprocal roots for the latency of one.
    const double a = d[0][0], b = d[1][0];
    const double det01 = fma(a, d[1][1], -(b * b));
    const double r0 = rsqrt_chain(a), rd01 = rsqrt_chain(det01);
    const double r1 = (a * r0) * rd01;
    const double l10 = b * r0, l20 = d[2][0] * r0, l30 = d[3][0] * r0;
    const double t21 = fma(-l20, l10, d[2][1]), t31 = fma(-l30, l10, d[3][1]);
    const double q22a = fma(-l20, l20, d[2][2]), q32a = fma(-l30, l20, d[3][2]), q33a = fma(-l30, l30, d[3][3]);
    const double l21 = t21 * r1, l31 = t31 * r1;
    const double p2 = fma(-l21, l21, q22a), t32 = fma(-l31, l21, q32a), q33b = fma(-l31, l31, q33a);
    const double det23 = fma(p2, q33b, -(t32 * t32));
    const double r2 = rsqrt_chain(p2), rd23 = rsqrt_chain(det23);
    const double r3 = (p2 * r2) * rd23;
    const double l32 = t32 * r2;
    // first non-positive (or NaN) pivot, 4 = none (pivot 1 = det01/a, pivot 3 = det23/p2); independent selects + min
    // instead of an early-exit chain, which the compiler turns into scalar branches in the middle of the chain
    const int b0 = a > 0.0 ? 4 : 0, b1 = det01 > 0.0 ? 4 : 1, b2 = p2 > 0.0 ? 4 : 2, b3 = det23 > 0.0 ? 4 : 3;
    bad = min(min(b0, b1), min(b2, b3));
    // inverse of the factor, row by row; each row's last multiply is by its own reciprocal root
    Inv44 w;
    w.w00 = r0;
    const double u10 = -l10 * r0;                     // w10 = u10 * r1
    w.w10 = u10 * r1; w.w11 = r1;
    const double l20r0 = l20 * r0;
    w.w20 = -fma(l21, w.w10, l20r0) * r2; w.w21 = -(l21 * r1) * r2; w.w22 = r2;
    const double s30 = fma(l31, w.w10, l30 * r0), s31 = l31 * r1;
    w.w30 = -fma(l32, w.w20, s30) * r3; w.w31 = -fma(l32, w.w21, s31) * r3; w.w32 = -(l32 * r2) * r3; w.w33 = r3;
    return w;
}

// One wave.  In: the lower triangle of the block at S[c0.., c0..].  Out: L^-1 -> the same block of S (the panel solve
// multiplies by its transpose), L^T tiles -> 12 staging rows of 64 doubles (flush_diag_block), first bad pivot -> badcol.
__device__ __forceinline__ void factor32_mfma(double* S, double* stage, int c0, int lane, int& badcol, long long* dbg = nullptr) {
    const int l15 = lane & 15, l4 = lane >> 4;
    int nst = 0;
    auto stamp = [&]() {
        if (dbg && lane == 0) dbg[nst] = (long long)__builtin_amdgcn_s_memtime();
        ++nst;
    };
    stamp();
    v4d T00, T01, T11, E00, E10, E11;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = l4 + 4 * r, col = l15;
        const int hi = row > col ? row : col, lo = row > col ? col : row;
        T00[r] = S[(c0 + hi) * SLD + c0 + lo];
        T01[r] = S[(c0 + 16 + col) * SLD + c0 + row];
        T11[r] = S[(c0 + 16 + hi) * SLD + c0 + 16 + lo];
        E00[r] = row == col ? 1.0 : 0.0;
        E11[r] = E00[r];
        E10[r] = 0.0;
    }
    stamp();
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    // lane (m, k) of the scaling MFMA's A operand carries inv[m][k] (m < 4, k <= m), zero elsewhere.  Bitwise select
    // with lane-constant masks: plain AND/OR on the pivot chain (a ternary chain here gets compiled into a
    // dynamically indexed private array, i.e. a scratch-memory round trip per step)
    auto lane_mask = [&](int m, int k) { return (l15 == m && l4 == k) ? ~0ull : 0ull; };
    const unsigned long long M00 = lane_mask(0, 0), M10 = lane_mask(1, 0), M11 = lane_mask(1, 1), M20 = lane_mask(2, 0),
                             M21 = lane_mask(2, 1), M22 = lane_mask(2, 2), M30 = lane_mask(3, 0), M31 = lane_mask(3, 1),
                             M32 = lane_mask(3, 2), M33 = lane_mask(3, 3);
    auto bits = [](double x) { return (unsigned long long)__double_as_longlong(x); };
    auto a_operand = [&](const Inv44& w) {
        const unsigned long long v = (bits(w.w00) & M00) | (bits(w.w10) & M10) | (bits(w.w11) & M11) | (bits(w.w20) & M20) |
                                     (bits(w.w21) & M21) | (bits(w.w22) & M22) | (bits(w.w30) & M30) | (bits(w.w31) & M31) |
                                     (bits(w.w32) & M32) | (bits(w.w33) & M33);
        return __longlong_as_double((long long)v);
    };
    // the scaled pivot rows (final rows of [L^T | L^-1]) are kept apart from the accumulators: nothing reads an
    // accumulator's pivot rows again (the update's A operand is zero there)
    double fT00[4], fT01[4], fE00[4], fT11[4], fE10[4], fE11[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // pivot rows 4q .. 4q+3 (row tile 0)
        int bad;
        const Inv44 w = inv_chol44(T00[q], 4 * q, bad);
        badcol = (badcol < 0 && bad < 4) ? c0 + 4 * q + bad : badcol;
        const double aw = a_operand(w);
        // the next pivot block lives in T00 (q < 3) or T11 (q == 3): its slab and its update go down the matrix pipe first
        const double sT0 = mfma_f64(aw, T00[q], zero)[0];
        const double a0 = l15 >= 4 * q + 4 ? -sT0 : 0.0;         // rows of tile 0 below the pivot rows
        if (q < 3) T00 = mfma_f64(a0, sT0, T00);
        __builtin_amdgcn_sched_barrier(0);                       // keep this pair ahead of the independent slabs
        const double sT1 = mfma_f64(aw, T01[q], zero)[0];
        const double a1 = -sT1;                                  // every row of tile 1
        if (q == 3) { T11 = mfma_f64(a1, sT1, T11); __builtin_amdgcn_sched_barrier(0); }
        const double sE0 = mfma_f64(aw, E00[q], zero)[0];
        fT00[q] = sT0; fT01[q] = sT1; fE00[q] = sE0;
        if (q < 3) {
            T01 = mfma_f64(a0, sT1, T01);
            E00 = mfma_f64(a0, sE0, E00);
            T11 = mfma_f64(a1, sT1, T11);
        }
        E10 = mfma_f64(a1, sE0, E10);
        stamp();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // pivot rows 16 + 4q .. (row tile 1)
        int bad;
        const Inv44 w = inv_chol44(T11[q], 4 * q, bad);
        badcol = (badcol < 0 && bad < 4) ? c0 + 16 + 4 * q + bad : badcol;
        const double aw = a_operand(w);
#ifdef EMCID_LEAF_MIDSTAMP
        stamp();
#endif
        const double sT1 = mfma_f64(aw, T11[q], zero)[0];
        const double a1 = l15 >= 4 * q + 4 ? -sT1 : 0.0;
        if (q < 3) T11 = mfma_f64(a1, sT1, T11);
        __builtin_amdgcn_sched_barrier(0);
        const double sE0 = mfma_f64(aw, E10[q], zero)[0];
        const double sE1 = mfma_f64(aw, E11[q], zero)[0];
        fT11[q] = sT1; fE10[q] = sE0; fE11[q] = sE1;
        if (q < 3) {
            E10 = mfma_f64(a1, sE0, E10);
            E11 = mfma_f64(a1, sE1, E11);
        }
        stamp();
    }
    // ---- outputs.  fT* hold L^T (valid for row <= col), fE* hold L^-1 (upper right tile = 0).
    stamp();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = l4 + 4 * r, col = l15;
        // L^-1 replaces the block in S (the panel solve reads it from there, transposed)
        S[(c0 + row) * SLD + c0 + col] = fE00[r];
        S[(c0 + row) * SLD + c0 + 16 + col] = 0.0;
        S[(c0 + 16 + row) * SLD + c0 + col] = fE10[r];
        S[(c0 + 16 + row) * SLD + c0 + 16 + col] = fE11[r];
    }
    stamp();
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // L^T tiles -> staging rows (lane-linear, conflict free); another wave takes them to global
        stage[(0 + r) * SLD + lane] = fT00[r];
        stage[(4 + r) * SLD + lane] = fT01[r];
        stage[(8 + r) * SLD + lane] = fT11[r];
    }
    stamp();
}

// second half of phase A's output, by a wave that is not on the pivot chain: L_pp -> global from the staged L^T tiles
// (L[i][j] = L^T[j][i]; a lane's four rows are adjacent columns of L; zeros above the diagonal)
__device__ __forceinline__ void flush_diag_block(const double* stage, int c0, double* __restrict__ L, int64_t ldl, int lane) {
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = l4 + 4 * r, col = l15;
        double* Lc = L + (int64_t)(c0 + col) * ldl + c0;
        Lc[row] = row <= col ? stage[(0 + r) * SLD + lane] : 0.0;
        Lc[16 + row] = 0.0;
        double* Lc1 = Lc + 16 * ldl;
        Lc1[row] = stage[(4 + r) * SLD + lane];
        Lc1[16 + row] = row <= col ? stage[(8 + r) * SLD + lane] : 0.0;
    }
}

constexpr int LEAF_LDS = NB * SLD + 2 * SB * ZLD;      // doubles

__device__ __forceinline__ void chol_leaf_body(const double* __restrict__ A, int64_t lda, double* __restrict__ L, int64_t ldl,
                                               double* __restrict__ inv, int64_t ldinv, int* info, int col0, long long* dbg,
                                               double* lds) {
    double* S = lds;
    constexpr int ZOFF = NB * SLD;          // two [32][48] temporaries behind S
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    int nstamp = 0;
    auto stamp = [&]() {   // diagnostic only (dbg != nullptr): shader-clock stamps of wave 0 at phase boundaries
        if (dbg && tid == 0) dbg[nstamp] = (long long)__builtin_amdgcn_s_memtime();
        ++nstamp;
    };
    stamp();

    {
        // 128 x 128 block = 8192 16-byte vectors, 16 per thread, fetched in batches of LEAF_LOAD_BATCH independent loads: the block
        // was written by other compute units in the launch before, so every batch pays a cold-read latency of its own
        constexpr int VPR = NB / 2;   // vectors per row
        constexpr int LB = LEAF_LOAD_BATCH;
#pragma unroll 1
        for (int b0 = 0; b0 < NB * VPR / LEAF_T; b0 += LB) {
            v2d x[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const int v = tid + (b0 + u) * LEAF_T;
                const int i = v / VPR, j = 2 * (v % VPR);
                x[u] = (j <= i) ? *reinterpret_cast<const v2d*>(A + (int64_t)i * lda + j) : (v2d){0.0, 0.0};
            }
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const int v = tid + (b0 + u) * LEAF_T;
                const int i = v / VPR, j = 2 * (v % VPR);
                if (j + 1 > i) x[u][1] = 0.0;   // strictly-upper element of a pair straddling the diagonal
                *reinterpret_cast<v2d*>(S + i * SLD + j) = x[u];
            }
        }
    }
    __syncthreads();
    stamp();

    int badcol = -1;   // first non-positive pivot seen by wave 0 (uniform)
#pragma unroll 1
    for (int p = 0; p < NB / SB; ++p) {
        const int c0 = p * SB;
        const int R0 = c0 + SB;               // first row below the diagonal block
        const int mb = (NB - R0) / 16;        // 16-row blocks below

        // ---- phase A: wave 0 factors the diagonal block and its inverse on the matrix pipe (factor32_mfma) ------------
        // staging rows: the never-touched upper right quadrant S[0:64][64:128] (12 rows per panel; lvl2 reuses it later)
        double* stage = S + (12 * p) * SLD + 64;
        if (wave == 0) factor32_mfma(S, stage, c0, lane, badcol, (dbg && p == 1) ? dbg + 16 : nullptr);
        __syncthreads();
        stamp();
        if (wave == LEAF_T / 64 - 1) flush_diag_block(stage, c0, L, ldl, lane);   // the last wave has the fewest panel rows
        if (mb == 0) break;

        // ---- phase B: P = A_below * Z (rows R0.., 32 columns), in place; one wave owns a 16-row block ---------
        for (int ib = wave; ib < mb; ib += LEAF_T / 64) {
            const int r0 = R0 + ib * 16;
            v4d acc[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
                acc[cb] = leaf_tile<SB>(lds, [&](int i, int k) { return (r0 + i) * SLD + c0 + k; },
                                        [&](int k, int j) { return (c0 + cb * 16 + j) * SLD + c0 + k; }, l15, l4);   // Z[k][c] = inv[c][k]
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = r0 + l4 + 4 * q, col = c0 + cb * 16 + l15;
                    S[row * SLD + col] = acc[cb][q];
                    L[(int64_t)row * ldl + col] = acc[cb][q];
                }
        }
        __syncthreads();
        stamp();

        // ---- phase C: trailing update T -= P P^T on the lower 16x16 tiles ---------------------------------------
        const int ntiles = mb * (mb + 1) / 2;
        for (int t = wave; t < ntiles; t += LEAF_T / 64) {
            int ib = 0, rem = t;
            while (rem > ib) { rem -= ib + 1; ++ib; }
            const int jb = rem;
            const int ri = R0 + ib * 16, rj = R0 + jb * 16;
            const v4d acc = leaf_tile<SB>(lds, [&](int i, int k) { return (ri + i) * SLD + c0 + k; },
                                          [&](int k, int j) { return (rj + j) * SLD + c0 + k; }, l15, l4);
#pragma unroll
            for (int q = 0; q < 4; ++q) S[(ri + l4 + 4 * q) * SLD + rj + l15] -= acc[q];
        }
        __syncthreads();
        stamp();
    }
    if (wave == 0 && lane == 0 && badcol >= 0) atomicCAS(info, 0, col0 + badcol + 1);  // not SPD (or NaN pivot)

    // ---- inverse assembly, level 1: the two 64-blocks.  X = -B (C A), A/B = 32x32 inverses, C = L block ------
    {
        constexpr int NW = LEAF_T / 64;
        // 8 tiles: (block q, tile ti, tj)
        for (int t = wave; t < 8; t += NW) {     // T1 = C A
            const int q = t >> 2, ti = (t >> 1) & 1, tj = t & 1, b = 64 * q, toff = ZOFF + q * SB * ZLD;
            const v4d acc = leaf_tile<SB>(lds, [&](int i, int k) { return (b + 32 + ti * 16 + i) * SLD + b + k; },
                                          [&](int k, int j) { return (b + k) * SLD + b + tj * 16 + j; }, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[toff + (ti * 16 + l4 + 4 * r) * ZLD + tj * 16 + l15] = acc[r];
        }
        __syncthreads();
        for (int t = wave; t < 8; t += NW) {     // X = -B T1, written over C
            const int q = t >> 2, ti = (t >> 1) & 1, tj = t & 1, b = 64 * q, toff = ZOFF + q * SB * ZLD;
            const v4d acc = leaf_tile<SB>(lds, [&](int i, int k) { return (b + 32 + ti * 16 + i) * SLD + b + 32 + k; },
                                          [&](int k, int j) { return toff + k * ZLD + tj * 16 + j; }, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(b + 32 + ti * 16 + l4 + 4 * r) * SLD + b + tj * 16 + l15] = -acc[r];
        }
        __syncthreads();
    }
    stamp();
    // ---- level 2: X64 = -B64 (C64 A64); T lives in the unused upper-right block S[0:64][64:128] ----------------
    for (int t = wave; t < 16; t += LEAF_T / 64) {
        const int ti = t >> 2, tj = t & 3;
        const v4d acc = leaf_tile<64>(lds, [&](int i, int k) { return (64 + ti * 16 + i) * SLD + k; },
                                      [&](int k, int j) { return k * SLD + tj * 16 + j; }, l15, l4);
#pragma unroll
        for (int r = 0; r < 4; ++r) S[(ti * 16 + l4 + 4 * r) * SLD + 64 + tj * 16 + l15] = acc[r];
    }
    __syncthreads();
    {
        v4d acc[(16 + LEAF_T / 64 - 1) / (LEAF_T / 64)];
        int n = 0;
        for (int t = wave; t < 16; t += LEAF_T / 64, ++n) {
            const int ti = t >> 2, tj = t & 3;
            acc[n] = leaf_tile<64>(lds, [&](int i, int k) { return (64 + ti * 16 + i) * SLD + 64 + k; },
                                   [&](int k, int j) { return k * SLD + 64 + tj * 16 + j; }, l15, l4);
        }
        __syncthreads();   // all reads of B64 / T done before C64's place is overwritten
        n = 0;
        for (int t = wave; t < 16; t += LEAF_T / 64, ++n) {
            const int ti = t >> 2, tj = t & 3;
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(64 + ti * 16 + l4 + 4 * r) * SLD + tj * 16 + l15] = -acc[n][r];
        }
    }
    __syncthreads();
    stamp();
    for (int v = tid; v < NB * NB / 2; v += LEAF_T) {
        const int i = v / (NB / 2), j = 2 * (v % (NB / 2));
        v2d x = *reinterpret_cast<const v2d*>(S + i * SLD + j);
        if (j > i) x[0] = 0.0;
        if (j + 1 > i) x[1] = 0.0;
        *reinterpret_cast<v2d*>(inv + (int64_t)i * ldinv + j) = x;
    }
    __syncthreads();
    stamp();
}

__global__ __launch_bounds__(LEAF_T) void chol_leaf_kernel(const double* __restrict__ A, int64_t lda, double* __restrict__ L,
                                                            int64_t ldl, double* __restrict__ inv, int64_t ldinv, int* info,
                                                            int col0, long long* dbg = nullptr, int64_t s_mat = 0,
                                                            int64_t s_inv = 0) {
    // blockIdx.x = which matrix of a batch (independent factorizations share the launch: their serial spines overlap)
    __shared__ __attribute__((aligned(16))) double lds[LEAF_LDS];
    chol_leaf_body(A + blockIdx.x * s_mat, lda, L + blockIdx.x * s_mat, ldl, inv + blockIdx.x * s_inv, ldinv, info, col0, dbg, lds);
}

// ---- what rides in the leaf launches: the ShadowJob and XrowJob of spd_solve.h ------------------------------------------------
static long long* g_step_stamps = nullptr;      // set by emcid_debug_step_stamps

template <int SH_BK, int SH_PF>
__device__ __forceinline__ void shadow_tile(const ShadowJob& sh, int bm, int bn, int slice, int nslices, double* smem) {
    using TA = OpTile<true, SH_BM, SH_BK>;
    using TB = OpTile<false, SH_BN, SH_BK>;
    GemmShape q{sh.A, sh.lda, sh.B, sh.ldb, sh.M, sh.N, sh.K, 0};
    q.tri = 2;
    q.nofast = sh.nofast;
    const int depth = streamk_depth(q, bn, SH_BN, SH_BK);
    const int per = (depth + nslices - 1) / nslices;
    const int kb = slice * per, ke = min(depth, kb + per);
    if (kb >= ke) return;
    constexpr int MI = SH_BM / 2 / 16, NI = SH_BN / 4 / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / 4) * (SH_BM / 2), wn0 = (wave % 4) * (SH_BN / 4);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int m0 = bm * SH_BM, n0 = bn * SH_BN;
    // The earlier slices' sum is fetched BEFORE the K loop (the launch before this one wrote it from another compute unit: a
    // cold read costs ~2.7 us here, scripts/step_stamps.py) and added after it; clamped addresses, so the loads are unconditional
    v4d prev[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = min(m0 + wm0 + TA::index_of(i, l4 + 4 * r), sh.M - 1);
                const int n = min(n0 + wn0 + TB::index_of(j, l15), sh.N - 1);
                prev[i][j][r] = slice ? sh.C[(int64_t)m * sh.ldc + n] : 0.0;
            }
    __builtin_amdgcn_sched_barrier(0);      // keep those loads up here
    v4d acc[MI][NI];
    gemm_f64_tile_acc<true, false, SH_BM, SH_BN, SH_BK, 2, 4, SH_PF>(q, bm, bn, smem, kb, ke, acc);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm0 + TA::index_of(i, l4 + 4 * r);
                const int n = n0 + wn0 + TB::index_of(j, l15);
                if (m < sh.M && n < sh.N) sh.C[(int64_t)m * sh.ldc + n] = prev[i][j][r] + acc[i][j][r];
            }
    __syncthreads();      // the next tile's first LDS store must not overtake this tile's last MFMA stage
}

// Both tiles of a pair in ONE software pipeline (interior shapes: M % 64 == N % 128 == K % 16 == 0): the K tiles of tile bn0's
// slice, then those of bn1's, flow through the same register ring and LDS double buffer; at the seam tile bn0's sum goes out
// while bn1's first K tiles are already in flight, so the second tile pays no load-latency prologue (~2.5 us of a 38 us launch).
__device__ __forceinline__ void shadow_pair_fused(const ShadowJob& sh, int bm, int bn0, int bn1, int slice, int nslices, double* smem) {
    constexpr int BK = 16, PF = 3, NT = LEAF_T;
    using TA = OpTile<true, SH_BM, BK>;
    using TB = OpTile<false, SH_BN, BK>;
    constexpr int STAGE = TA::SIZE + TB::SIZE;
    constexpr int MI = SH_BM / 2 / 16, NI = SH_BN / 4 / 16;
    constexpr int NA = TA::NVEC / NT, NB = TB::NVEC / NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / 4) * (SH_BM / 2), wn0 = (wave % 4) * (SH_BN / 4);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int m0 = bm * SH_BM;
    const int KT = sh.K / BK;
    // segment g: column tile bn[g], absolute K tiles [kb[g], ke[g])  (B(k, n) = 0 for k < n: the tile's own range starts at its column)
    int bn[2] = {bn0, bn1}, kb[2], ke[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int first = bn[g] * SH_BN / BK, depth = KT - first;
        const int per = (depth + nslices - 1) / nslices;
        kb[g] = first + min(depth, slice * per);
        ke[g] = first + min(depth, slice * per + per);
    }
    const int n0len = ke[0] - kb[0], total = n0len + (ke[1] - kb[1]);
    if (total <= 0) return;
    const double* pa[NA];
    const double* pb[NB];
    int la[NA], lb[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int v = tid + i * NT;
        pa[i] = sh.A + (int64_t)(m0 + v / (BK / 2)) * sh.lda + 2 * (v % (BK / 2));
        la[i] = (v / (BK / 2)) * TA::LD + 2 * (v % (BK / 2));
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int v = tid + i * NT;
        pb[i] = sh.B + (int64_t)(v / (SH_BN / 2)) * sh.ldb + 2 * (v % (SH_BN / 2));
        lb[i] = (v / (SH_BN / 2)) * TB::LD + 2 * (v % (SH_BN / 2));
    }
    v2d fa[PF][NA], fb[PF][NB];
    auto fetch = [&](int s, int u) {            // unified step u -> (segment, absolute K tile); past the end: the last one again
        const int uu = u < total ? u : total - 1;
        const int g = uu < n0len ? 0 : 1;
        const int64_t kt = g ? kb[1] + (uu - n0len) : kb[0] + uu;
        const int64_t ncol = (int64_t)bn[g] * SH_BN;
#pragma unroll
        for (int i = 0; i < NA; ++i) fa[s][i] = *reinterpret_cast<const v2d*>(pa[i] + kt * BK);
#pragma unroll
        for (int i = 0; i < NB; ++i) fb[s][i] = *reinterpret_cast<const v2d*>(pb[i] + kt * BK * sh.ldb + ncol);
    };
    auto stash = [&](int s, double* stage) {
#pragma unroll
        for (int i = 0; i < NA; ++i) *reinterpret_cast<v2d*>(stage + la[i]) = fa[s][i];
#pragma unroll
        for (int i = 0; i < NB; ++i) *reinterpret_cast<v2d*>(stage + TA::SIZE + lb[i]) = fb[s][i];
    };
    v4d prev[MI][NI], acc[MI][NI];
    auto c_ptr = [&](int g, int i, int j, int r) {
        return sh.C + (int64_t)(m0 + wm0 + TA::index_of(i, l4 + 4 * r)) * sh.ldc + bn[g] * SH_BN + wn0 + TB::index_of(j, l15);
    };
    auto load_prev = [&](int g) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) prev[i][j][r] = slice ? *c_ptr(g, i, j, r) : 0.0;
    };
    auto flush = [&](int g) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    *c_ptr(g, i, j, r) = prev[i][j][r] + acc[i][j][r];
                    acc[i][j][r] = 0.0;
                }
    };
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    load_prev(n0len > 0 ? 0 : 1);
#pragma unroll
    for (int s = 0; s < PF; ++s) fetch(s, s);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    stash(0, smem);
    __syncthreads();
    for (int base = 0; base < total; base += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            const int u = base + s;
            if (u < total) {
                const double* As = smem + (u & 1) * STAGE;
                const double* Bs = As + TA::SIZE;
                fetch(s, u + PF);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k8 = 0; k8 < BK / 8; ++k8) {
                    double a[2][MI], b[2][NI];
                    TA::template frags<MI>(As, wm0, k8, l15, l4, a);
                    TB::template frags<NI>(Bs, wn0, k8, l15, l4, b);
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int i = 0; i < MI; ++i)
#pragma unroll
                            for (int j = 0; j < NI; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e][i], b[e][j], acc[i][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (u + 1 < total) stash((s + 1) % PF, smem + ((u + 1) & 1) * STAGE);
                if (u + 1 == n0len && n0len < total) {       // the seam: tile bn0 is complete, bn1's K tiles are already in flight
                    flush(0);
                    load_prev(1);
                }
                __syncthreads();
            }
        }
    }
    flush(n0len < total ? 1 : 0);
    __syncthreads();
}

template <int SH_BK, int SH_PF>
__device__ __forceinline__ void shadow_pair(const ShadowJob& sh, int s_, int slice, int nslices, double* lds) {
    const int ntl = (sh.N + SH_BN - 1) / SH_BN, npairs = (ntl + 1) / 2;
    int bm = s_ / npairs, pr = s_ % npairs;
    if (sh.xcd_gx > 0) {
        // The workgroups of a launch go to the 8 XCDs round-robin by id, so shadow workgroups s_ = g (mod 8) share an L2.  Give
        // each XCD a compact gx x gy block of the (row tile, column pair) grid: its 24 workgroups then re-read each other's A and
        // B tiles out of their own L2 (B: half of the X slice, 2.4 MB at d = 3072) instead of all 192 streaming everything from
        // the Infinity Cache — the K loop here is bound by that traffic, not by the matrix pipe (scripts/step_stamps.py).
        const int mb = (sh.M + SH_BM - 1) / SH_BM;
        const int g = s_ & 7, r = s_ >> 3;
        const int gy = 8 / sh.xcd_gx, rows = mb / sh.xcd_gx, cols = npairs / gy;
        bm = (g / gy) * rows + r / cols;
        pr = (g % gy) * cols + r % cols;
    }
    if (SH_BK == 16 && SH_PF == 3 && sh.fuse_pair && ntl - 1 - pr != pr && sh.M % SH_BM == 0 && sh.N % SH_BN == 0 &&
        sh.K % SH_BK == 0) {
        shadow_pair_fused(sh, bm, pr, ntl - 1 - pr, slice, nslices, lds);
        return;
    }
    shadow_tile<SH_BK, SH_PF>(sh, bm, pr, slice, nslices, lds);                            // the long K range first
    if (ntl - 1 - pr != pr) shadow_tile<SH_BK, SH_PF>(sh, bm, ntl - 1 - pr, slice, nslices, lds);
}

// One launch = the leaf of block j (workgroup 0) AND the trailing update of step j-1 that the leaf does not depend on (the other
// workgroups, one 128 x 128 tile each): on one in-order stream a leaf and the previous step's bulk cannot overlap as two kernels,
// and as parallel graph branches they cost more than they save (see cholesky_impl) — as one grid they simply run side by side.
// Behind those, sh.wgs workgroups of the caller's shadow product (slice `slice` of `nslices`).
__global__ __launch_bounds__(LEAF_T) void chol_step_leaf_kernel(const double* __restrict__ A, int64_t lda, double* __restrict__ L,
                                                                 int64_t ldl, double* __restrict__ inv, int64_t ldinv, int* info,
                                                                 int col0, GemmShape trail, EpiAxpby trail_epi, int ntrail,
                                                                 ShadowJob sh, int slice, int nslices, GemmShape xr, EpiAxpby xr_epi,
                                                                 int nxr) {
    __shared__ __attribute__((aligned(16))) double lds[LEAF_LDS];
    long long* stamp = (sh.stamps && blockIdx.x < 512) ? sh.stamps + ((int64_t)slice * 512 + blockIdx.x) * 4 : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = (long long)__builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0) {
        chol_leaf_body(A, lda, L, ldl, inv, ldinv, info, col0, nullptr, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 1; }
        return;
    }
    if ((int)blockIdx.x <= ntrail) {
        // lower-trapezoid tile (bm, bn), bn <= bm + 1, from the linear index: row bm holds bm + 2 tiles
        int bm = 0, rem = (int)blockIdx.x - 1;
        while (rem >= bm + 2) { rem -= bm + 2; ++bm; }
        gemm_f64_tile<true, true, 128, 128, 16, 2, 4, EpiAxpby>(trail, trail_epi, bm, rem, 0, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 2; }
        return;
    }
    if ((int)blockIdx.x <= ntrail + nxr) {      // a 32 x 64 tile of Tt = Xt L[j, 0:j]^T (XrowJob) on the workgroup's first four waves
        // (a 128 x 128 tile of it contracts up to 896 deep on ONE compute unit: ~100 us, three leaf launches long; the small tiles
        // finish under the leaf, and 8 j of them still leave every shadow workgroup a compute unit of its own)
        if (threadIdx.x >= 256) return;
        const int t = (int)blockIdx.x - 1 - ntrail;
        gemm_f64_tile<true, true, 32, 64, 16, 2, 2, EpiAxpby>(xr, xr_epi, t / 2, t % 2, 0, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 6; }
        return;
    }
    ntrail += nxr;
    int s_ = (int)blockIdx.x - 1 - ntrail;
    // (K-tile depth 32, 6 or 8 K tiles of loads in flight and LDS fragment prefetch were measured here as template variants:
    //  none moved the launch time by more than 1 us)
    shadow_pair<16, 3>(sh, s_, slice, nslices, lds);
    if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 3; }
}


// ---- the step between two leaves of a small Cholesky: L[j+1, j] and the next diagonal block -------------------------------------
// After leaf j the next leaf needs exactly one 128 x 128 block: D = A[j+1, j+1] - P P^T with P = L[j+1, j] = A[j+1, j] inv(L_jj)^T.
// As two launches of the tile GEMM this costs ~17 us of latency on the serial spine of the factorization; here it is one
// launch of 36 workgroups, one per lower 16 x 16 tile (bi, bj) of D: the workgroup forms the two 16-row strips P_i and P_j it
// needs itself (redundantly — no workgroup waits for another), updates its tile, and the bj == 0 column also stores its P_i
// strip into L.  Operands through LDS with the leaf's row stride; the triangular inverse is staged in two 64-row halves.
constexpr int SP_T = 256;
constexpr int SP_R = 16;                    // strip height
constexpr int SP_LDS = (64 + 4 * SP_R) * SLD;

template <class FA, class FB>
__device__ __forceinline__ v4d leaf_tile_k(const double* lds, FA fa, FB fb, int l15, int l4, int K) {
    v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < K / 4; kk += 2) {
        const double a0 = lds[fa(l15, kk * 4 + l4)];
        const double b0 = lds[fb(kk * 4 + l4, l15)];
        const double a1 = lds[fa(l15, kk * 4 + 4 + l4)];
        const double b1 = lds[fb(kk * 4 + 4 + l4, l15)];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

__device__ __forceinline__ void chol_spine_body(const double* __restrict__ Ablk, int64_t lda, const double* __restrict__ inv, int64_t ldi,
                                                double* __restrict__ Lout, int64_t ldl, double* __restrict__ D, int tile, double* lds) {
    double* sInv = lds;                     // [64][SLD]   half of inv(L_jj): rows n of the half, columns k
    double* sAi = lds + 64 * SLD;           // [16][SLD]   A strips
    double* sAj = sAi + SP_R * SLD;
    double* sPi = sAj + SP_R * SLD;
    double* sPj = sPi + SP_R * SLD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // lower tile (bi, bj) of the 8 x 8 tiles of D from the linear tile index
    int bi = 0, rem = tile;
    while (rem > bi) { rem -= bi + 1; ++bi; }
    const int bj = rem;
    // every global vector this thread will stage, fetched up front (32 independent 16-byte loads: the two A strips, the
    // 64 x 64 and the 64 x 128 halves of the triangular inverse), so the kernel pays ONE memory latency, not one per vector
    v2d ra[8], r0[8], r1[16];
    double dold[4];         // the D tile as it is (wave 0 subtracts from it at the very end: fetched NOW, not then — a cold read is ~2.5 us)
#pragma unroll
    for (int q = 0; q < 4; ++q) dold[q] = D[(int64_t)(bi * SP_R + l4 + 4 * q) * lda + bj * SP_R + l15];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int v = tid + u * SP_T;                               // 2 strips x 16 rows x 64 vectors
        const int which = v / (SP_R * (NB / 2)), w = v % (SP_R * (NB / 2));
        const int r = w / (NB / 2), c = 2 * (w % (NB / 2));
        ra[u] = *reinterpret_cast<const v2d*>(Ablk + (int64_t)((which ? bj : bi) * SP_R + r) * lda + c);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int v = tid + u * SP_T;                               // 64 rows x 32 vectors
        r0[u] = *reinterpret_cast<const v2d*>(inv + (int64_t)(v / 32) * ldi + 2 * (v % 32));
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int v = tid + u * SP_T;                               // 64 rows x 64 vectors
        r1[u] = *reinterpret_cast<const v2d*>(inv + (int64_t)(64 + v / 64) * ldi + 2 * (v % 64));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int v = tid + u * SP_T;
        const int which = v / (SP_R * (NB / 2)), w = v % (SP_R * (NB / 2));
        *reinterpret_cast<v2d*>((which ? sAj : sAi) + (w / (NB / 2)) * SLD + 2 * (w % (NB / 2))) = ra[u];
    }
    for (int half = 0; half < 2; ++half) {
        __syncthreads();                    // previous half's reads done
        if (half == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int v = tid + u * SP_T;
                *reinterpret_cast<v2d*>(sInv + (v / 32) * SLD + 2 * (v % 32)) = r0[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int v = tid + u * SP_T;
                *reinterpret_cast<v2d*>(sInv + (v / 64) * SLD + 2 * (v % 64)) = r1[u];
            }
        }
        __syncthreads();
        // P[:, 16 t .. 16 t + 16] = A[:, 0 : K] inv[16 t .., 0 : K]^T with K = 16 (t + 1): four column tiles per half, one per
        // wave — the deeper tiles of the second half go to the waves that had the shallow ones in the first
        const int tl = half ? 3 - wave : wave;          // tile inside the half
        const int t = 4 * half + tl, K = SP_R * (t + 1);
        // P_i and P_j tiles in ONE loop: they share the inverse fragment (B operand), and four independent accumulator chains
        // cover the LDS latency that two chains per call left exposed (stamps: a spine workgroup was 12.5 us, 5 of them here)
        v4d pi0 = {0.0, 0.0, 0.0, 0.0}, pi1 = pi0, pj0 = pi0, pj1 = pi0;
        {
            const double* ai = sAi + l15 * SLD + l4;
            const double* aj = sAj + l15 * SLD + l4;
            const double* bb = sInv + (tl * SP_R + l15) * SLD + l4;
            for (int k = 0; k < K; k += 16) {       // K is a multiple of 16: two 8-deep steps per trip, all twelve reads up front
                const double b0 = bb[k], b1 = bb[k + 4], b2 = bb[k + 8], b3 = bb[k + 12];
                const double x0 = ai[k], x1 = ai[k + 4], x2 = ai[k + 8], x3 = ai[k + 12];
                const double y0 = aj[k], y1 = aj[k + 4], y2 = aj[k + 8], y3 = aj[k + 12];
                pi0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, b0, pi0, 0, 0, 0);
                pj0 = __builtin_amdgcn_mfma_f64_16x16x4f64(y0, b0, pj0, 0, 0, 0);
                pi1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, b1, pi1, 0, 0, 0);
                pj1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y1, b1, pj1, 0, 0, 0);
                pi0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, b2, pi0, 0, 0, 0);
                pj0 = __builtin_amdgcn_mfma_f64_16x16x4f64(y2, b2, pj0, 0, 0, 0);
                pi1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x3, b3, pi1, 0, 0, 0);
                pj1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y3, b3, pj1, 0, 0, 0);
            }
        }
        const v4d pi = pi0 + pi1, pj = pj0 + pj1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sPi[(l4 + 4 * q) * SLD + t * SP_R + l15] = pi[q];
            sPj[(l4 + 4 * q) * SLD + t * SP_R + l15] = pj[q];
        }
    }
    __syncthreads();
    // ---- D tile -= P_i P_j^T, the 128-deep contraction cut over the four waves and summed through LDS (sInv is free now)
    {
        const int k0 = 32 * wave;
        const v4d part = leaf_tile_k(lds, [&](int i, int k) { return (int)(sPi - lds) + i * SLD + k0 + k; },
                                     [&](int k, int j) { return (int)(sPj - lds) + j * SLD + k0 + k; }, l15, l4, 32);
#pragma unroll
        for (int q = 0; q < 4; ++q) sInv[(wave * SP_R + l4 + 4 * q) * SLD + l15] = part[q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = l4 + 4 * q;
            const double sum = (sInv[r * SLD + l15] + sInv[(SP_R + r) * SLD + l15]) + (sInv[(2 * SP_R + r) * SLD + l15] + sInv[(3 * SP_R + r) * SLD + l15]);
            D[(int64_t)(bi * SP_R + r) * lda + bj * SP_R + l15] = dold[q] - sum;
        }
    }
    if (bj == 0) {      // this column of workgroups covers every strip once: P_i -> L[j+1, j]
        for (int v = tid; v < SP_R * (NB / 2); v += SP_T) {
            const int r = v / (NB / 2), c = 2 * (v % (NB / 2));
            *reinterpret_cast<v2d*>(Lout + (int64_t)(bi * SP_R + r) * ldl + c) = *reinterpret_cast<const v2d*>(sPi + r * SLD + c);
        }
    }
}

// One launch = the spine step of block j (workgroups 0..35) AND the rest of panel j (32 x 64 tiles of L[j+2.., j] = A[j+2.., j]
// inv(L_jj)^T): both need leaf j only, neither needs the other.
__global__ __launch_bounds__(SP_T) void chol_step_spine_kernel(const double* __restrict__ Ablk, int64_t lda, const double* __restrict__ inv,
                                                                int64_t ldi, double* __restrict__ Lout, int64_t ldl, double* __restrict__ D,
                                                                GemmShape panel, EpiAxpby panel_epi, long long* stamps, int step,
                                                                int npanel, GemmShape xs, EpiAxpby xs_epi, int nxs, double* xdiag,
                                                                int64_t ldxd) {
    __shared__ __attribute__((aligned(16))) double lds[SP_LDS];
    // diagnostic (stamps usually null): [start, -, end, kind] per workgroup behind the leaf launches' table (kind 4 spine, 5 panel)
    long long* stamp = (stamps && blockIdx.x < 512) ? stamps + ((int64_t)(16 + step) * 512 + blockIdx.x) * 4 : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = (long long)__builtin_amdgcn_s_memrealtime();
    if (blockIdx.x < 36) {
        chol_spine_body(Ablk, lda, inv, ldi, Lout, ldl, D, (int)blockIdx.x, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 4; }
        return;
    }
    int t = (int)blockIdx.x - 36;
    if (t < npanel) {
        gemm_f64_tile<true, true, 32, 64, 16, 2, 2, EpiAxpby>(panel, panel_epi, t / 2, t % 2, 0, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 5; }
        return;
    }
    t -= npanel;
    if (t < nxs) {                              // XrowJob: Xt[0:128j, j] = -Tt inv(L_jj)^T
        gemm_f64_tile<true, true, 32, 64, 16, 2, 2, EpiAxpby>(xs, xs_epi, t / 2, t % 2, 0, lds);
        if (stamp && threadIdx.x == 0) { stamp[2] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[3] = 7; }
        return;
    }
    if (xdiag != nullptr)                       // XrowJob: Xt[j, j] = inv(L_jj)^T, zeros below its diagonal
        for (int v = threadIdx.x; v < NB * NB; v += SP_T) {
            const int r = v / NB, c = v % NB;
            xdiag[(int64_t)r * ldxd + c] = (r <= c) ? inv[(int64_t)c * ldi + r] : 0.0;
        }
}

// the same transposed copy as a launch of its own (behind the last leaf there is no spine launch)
__global__ __launch_bounds__(256) void copy_inverse_transposed_kernel(const double* __restrict__ inv, int64_t ldi, double* __restrict__ xdiag,
                                                                       int64_t ldxd) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < NB * NB; v += gridDim.x * 256) {
        const int r = v / NB, c = v % NB;
        xdiag[(int64_t)r * ldxd + c] = (r <= c) ? inv[(int64_t)c * ldi + r] : 0.0;
    }
}

// ---- host orchestration -------------------------------------------------------------------------------

// invw: [ceil(dp/OB)] x (OB*OB inverse block, ld OB) followed by ceil(dp/OB) x (TB*TB scratch)
static inline double* inv_block(double* invw, int64_t J) { return invw + J * (int64_t)OB * OB; }
static inline const double* inv_block(const double* invw, int64_t J) { return invw + J * (int64_t)OB * OB; }

// Completes inv(L_JJ) for every OB x OB diagonal block from the leaf's 128 x 128 inverses, two levels of
//   inv([[A,0],[C,B]]) = [[A^-1, 0], [-B^-1 C A^-1, B^-1]]      (batched over the blocks)
static void build_block_inverses(const double* L, int64_t dp, int64_t lda, double* invw, hipStream_t st, int nmat = 1,
                                 int64_t s_mat = 0, int64_t s_inv = 0) {
    // nmat matrices (strides s_mat for L, s_inv for their inverse workspaces) share every launch: the products are
    // batched over the diagonal blocks AND over the matrices (GemmShape.batch2)
    const int64_t nob = (dp + OB - 1) / OB, nfull = dp / OB, rem = dp % OB;
    double* tmp = invw + nob * (int64_t)OB * OB;
    auto product = [&](const double* A, int64_t ldA, int64_t sA, int64_t sA2, bool b_lower, const double* B, int64_t ldB,
                       int64_t sB, int64_t sB2, double* C, int64_t ldC, int64_t sC, int64_t sC2, int M, int N, int K,
                       double alpha, int cnt) {
        GemmShape p{A, ldA, B, ldB, M, N, K, 0, sA, sB, cnt};
        p.sA2 = sA2; p.sB2 = sB2; p.batch2 = nmat;
        p.tri = b_lower ? 2 : 0;   // B stored [k][n] and lower triangular: zero for k < n
        EpiAxpby e{C, ldC, alpha, 0.0, sC};
        e.sC2 = sC2;
        launch_gemm_f64<true, false>(p, e, st, 2);
    };
    ScopedProf sp(KC_INV_BLOCK, st);
    const int64_t sI = (int64_t)OB * OB, sT = (int64_t)TB * TB, sL = (int64_t)OB * lda + OB;
    // level a: 256-blocks from pairs of 128-inverses.  u selects the pair inside an OB block.  ONE matrix with whole OB blocks
    // only (the N x N system of the dual solver at N = 1000): its second batch dimension is free, so the two pairs of every
    // block share a launch (two launches instead of four on the tail behind the last leaf, ~8 us each).
    if (nmat == 1 && rem == 0 && nfull > 0) {
        const int64_t hopL = 2 * NB * (lda + 1), hopI = 2 * NB * (int64_t)(OB + 1), hopT = (int64_t)NB * TB;
        const double* Cb = L + (int64_t)NB * lda;
        double* Ai = inv_block(invw, 0);
        double* Bi = inv_block(invw, 0) + NB * (int64_t)(OB + 1);
        double* X = inv_block(invw, 0) + NB * (int64_t)OB;
        GemmShape p1{Cb, lda, Ai, OB, NB, NB, NB, 0, sL, sI, (int)nfull};
        p1.sA2 = hopL; p1.sB2 = hopI; p1.batch2 = 2;
        p1.tri = 2;
        EpiAxpby e1{tmp, TB, 1.0, 0.0, sT};
        e1.sC2 = hopT;
        launch_gemm_f64<true, false>(p1, e1, st, 2);                                                 // T = C A^-1
        GemmShape p2{Bi, OB, tmp, TB, NB, NB, NB, 0, sI, sT, (int)nfull};
        p2.sA2 = hopI; p2.sB2 = hopT; p2.batch2 = 2;
        EpiAxpby e2{X, OB, -1.0, 0.0, sI};
        e2.sC2 = hopI;
        launch_gemm_f64<true, false>(p2, e2, st, 2);                                                 // X = -B^-1 T
    } else
    for (int u = 0; u < 2; ++u) {
        auto level_a = [&](int64_t J0, int cnt) {
            const double* Cb = L + ((J0 * 4 + 2 * u + 1) * NB) * lda + (J0 * 4 + 2 * u) * NB;
            double* Ai = inv_block(invw, J0) + (2 * u * NB) * (int64_t)(OB + 1);
            double* Bi = inv_block(invw, J0) + ((2 * u + 1) * NB) * (int64_t)(OB + 1);
            double* X = inv_block(invw, J0) + ((2 * u + 1) * NB) * (int64_t)OB + 2 * u * NB;
            double* T = tmp + J0 * sT;
            product(Cb, lda, sL, s_mat, true, Ai, OB, sI, s_inv, T, TB, sT, s_inv, NB, NB, NB, 1.0, cnt);      // T = C A^-1
            product(Bi, OB, sI, s_inv, false, T, TB, sT, s_inv, X, OB, sI, s_inv, NB, NB, NB, -1.0, cnt);      // X = -B^-1 T
        };
        if (nfull > 0) level_a(0, (int)nfull);
        if (rem >= (u + 1) * 2 * NB) level_a(nfull, 1);
    }
    // level b: the OB block from its two 256-halves (the lower half may be short in the last block)
    auto level_b = [&](int64_t J0, int cnt, int mrows) {
        const double* Cb = L + ((J0 * 4 + 2) * NB) * lda + (J0 * 4) * NB;
        double* Ai = inv_block(invw, J0);
        double* Bi = inv_block(invw, J0) + (2 * NB) * (int64_t)(OB + 1);
        double* X = inv_block(invw, J0) + (2 * NB) * (int64_t)OB;
        double* T = tmp + J0 * sT;
        product(Cb, lda, sL, s_mat, true, Ai, OB, sI, s_inv, T, TB, sT, s_inv, mrows, 2 * NB, 2 * NB, 1.0, cnt);
        product(Bi, OB, sI, s_inv, false, T, TB, sT, s_inv, X, OB, sI, s_inv, mrows, 2 * NB, mrows, -1.0, cnt);
    };
    if (nfull > 0) level_b(0, (int)nfull, 2 * NB);
    if (rem > 2 * NB) level_b(nfull, 1, (int)(rem - 2 * NB));
}

// Two-level blocked Cholesky on one stream.  Outer blocks of OB = 512 columns are brought up to date LEFT-looking
// (one GEMM against all previous columns, contraction depth = their count, so the Schur complement is read and
// written once per 512 columns instead of once per 128); inside an outer block the classic right-looking
// leaf -> panel -> trailing-update runs with NB = 128, its updates confined to the block's own <= 384 remaining columns.
int cholesky_serial(double* A, double* L, int64_t dp, int64_t lda, double* invw, int* info, hipStream_t st, int nbatch,
                    int64_t s_mat, int64_t s_inv) {
    // nbatch independent matrices (A + b*s_mat, L + b*s_mat, invw + b*s_inv; s_inv == inv_doubles(dp)) are factored by
    // the same launches: every GEMM is batched over blockIdx.z and the leaf runs one workgroup per matrix.
    hipLaunchKernelGGL(zero_f64_kernel, dim3(1024), dim3(256), 0, st, invw, inv_doubles(dp) * nbatch);
    const int nob = (int)((dp + OB - 1) / OB);
    for (int J = 0; J < nob; ++J) {
        const int64_t c0 = (int64_t)J * OB;
        const int w = (int)((dp - c0) < OB ? (dp - c0) : OB);
        if (J > 0) {
            // A[c0:, c0:c0+w] -= L[c0:, 0:c0] L[c0:c0+w, 0:c0]^T   (its top-left corner is on the diagonal)
            const double* Lr = L + c0 * lda;
            GemmShape g{Lr, lda, Lr, lda, (int)(dp - c0), w, (int)c0, 1, s_mat, s_mat, nbatch};
            ScopedProf sp(KC_CHOL_TRAIL, st);
            launch_gemm_f64<true, true>(g, EpiAxpby{A + c0 * lda + c0, lda, -1.0, 1.0, s_mat}, st);
        }
        for (int jj = 0; jj < w / NB; ++jj) {
            const int64_t o = c0 + (int64_t)jj * NB;
            double* inv = inv_block(invw, J) + (jj * NB) * (int64_t)(OB + 1);
            {
                ScopedProf sp(KC_CHOL_LEAF, st);
                hipLaunchKernelGGL(chol_leaf_kernel, dim3(nbatch), dim3(LEAF_T), 0, st, A + o * lda + o, lda, L + o * lda + o,
                                   lda, inv, (int64_t)OB, info, (int)o, (long long*)nullptr, s_mat, s_inv);
            }
            const int m = (int)(dp - o - NB);
            if (m == 0) break;
            GemmShape ps{A + (o + NB) * lda + o, lda, inv, OB, m, NB, NB, 0, s_mat, s_inv, nbatch};
            ps.tri = 1;   // inv(L11) is lower triangular: B(k, n) = inv[n][k] vanishes for k > n
            {
                ScopedProf sp(KC_CHOL_PANEL, st);
                launch_gemm_f64<true, true>(ps, EpiAxpby{L + (o + NB) * lda + o, lda, 1.0, 0.0, s_mat}, st);
            }
            const int wi = (int)(c0 + w - (o + NB));   // columns of this outer block still to the right
            if (wi > 0) {
                const double* L21 = L + (o + NB) * lda + o;
                GemmShape ts{L21, lda, L21, lda, m, wi, NB, 1, s_mat, s_mat, nbatch};
                ScopedProf sp(KC_CHOL_INNER, st);
                launch_gemm_f64<true, true>(ts, EpiAxpby{A + (o + NB) * lda + (o + NB), lda, -1.0, 1.0, s_mat}, st);
            }
        }
    }
    build_block_inverses(L, dp, lda, invw, st, nbatch, s_mat, s_inv);
    return check_launch("emcid_cholesky_f64");
}

// ---- small Cholesky, two heterogeneous launches per 128 columns (n <= 2048) -------------------------------------------------------
// Step j:   launch A_j = { leaf j }  +  { trailing update of step j-1 minus the block the leaf needs }
//           launch B_j = { spine step j: L[j+1, j] and the next diagonal block }  +  { the rest of panel j }
// Everything a launch contains depends on earlier LAUNCHES only, so the parts run side by side on the chip and the serial chain
// per step is leaf + spine step + two kernel boundaries (~48 us) instead of leaf + panel + trailing update + three (~65 us) — with
// one stream, i.e. without parallel graph branches (see cholesky_impl).
static int cholesky_fused_steps(double* A, double* L, int64_t n, int64_t lda, double* invw, int* info, hipStream_t st,
                                const ShadowJob* shadow, const XrowJob* xrow) {
    const int nb = (int)(n / NB);
    hipLaunchKernelGGL(zero_f64_kernel, dim3(1024), dim3(256), 0, st, invw, inv_doubles(n));
    for (int j = 0; j < nb; ++j) {
        const int64_t o = (int64_t)j * NB;
        double* inv = inv_block(invw, j / 4) + ((j % 4) * NB) * (int64_t)(OB + 1);
        {   // A_j
            const int M = (j >= 1) ? (int)(n - o - NB) : 0;           // rows j+1.. still to be updated by column j-1
            GemmShape tr{L, lda, L, lda, 0, 0, NB, 1};
            EpiAxpby te{A, lda, -1.0, 1.0};
            int ntiles = 0;
            if (M > 0) {
                tr = GemmShape{L + (o + NB) * lda + (o - NB), lda, L + o * lda + (o - NB), lda, M, M + NB, NB, 1};
                tr.lower_shift = NB;
                te.C = A + (o + NB) * lda + o;
                const int Mb = M / NB;
                ntiles = Mb * (Mb + 3) / 2;
            }
            ShadowJob sh{};
            if (shadow) sh = *shadow;
            sh.stamps = g_step_stamps;
            sh.xcd_gx = 0;
            sh.nofast = 0;
            sh.fuse_pair = 1;
            if (sh.wgs && sh.wgs % 8 == 0) {
                const int mb = (sh.M + SH_BM - 1) / SH_BM, np_ = ((sh.N + SH_BN - 1) / SH_BN + 1) / 2;
                // (shadow ids with the same s_ % 8 land on the same XCD whatever the id of the first one is)
                for (int gx : {4, 2, 8, 1})
                    if (mb % gx == 0 && np_ % (8 / gx) == 0) { sh.xcd_gx = gx; break; }
            }
            const int shadow_ids = sh.wgs;
            // XrowJob: Tt = Xt[0:o, 0:o] L[j, 0:j]^T on 32 x 64 tiles (K range from the tile's own first row on: X is lower
            // triangular, Xt upper)
            GemmShape xr{L, lda, L, lda, 0, 0, NB, 0};
            EpiAxpby xe{A, lda, 1.0, 0.0};
            int nxr = 0;
            if (xrow && j >= 1) {
                xr = GemmShape{xrow->Xt, xrow->ldx, L + o * lda, lda, (int)o, NB, (int)o, 0};
                xr.tri = 8;
                xr.pf = 1;
                xe = EpiAxpby{xrow->Tt, NB, 1.0, 0.0};
                nxr = (int)(o / 32) * 2;
            }
            ScopedProf sp(KC_CHOL_LEAF, st);
            hipLaunchKernelGGL(chol_step_leaf_kernel, dim3(1 + ntiles + nxr + shadow_ids), dim3(LEAF_T), 0, st, A + o * lda + o, lda,
                               L + o * lda + o, lda, inv, (int64_t)OB, info, (int)o, tr, te, ntiles, sh, j, nb, xr, xe, nxr);
        }
        if (j == nb - 1) {
            if (xrow) {     // the last block row of X: its second product and its diagonal block, no spine launch to ride in
                ScopedProf sp(KC_INV_BLOCK, st);
                GemmShape g{xrow->Tt, NB, inv, OB, (int)o, NB, NB, 0};
                g.tri = 1;      // B(k, n) = inv[n][k], zero for k > n
                launch_gemm_f64<true, true>(g, EpiAxpby{xrow->Xt + o, xrow->ldx, -1.0, 0.0}, st, 2);
                hipLaunchKernelGGL(copy_inverse_transposed_kernel, dim3(16), dim3(256), 0, st, inv, (int64_t)OB,
                                   xrow->Xt + o * xrow->ldx + o, xrow->ldx);
            }
            break;
        }
        {   // B_j
            const int m2 = (int)(n - o - 2 * NB);
            GemmShape ps{A, lda, inv, OB, 0, NB, NB, 0};
            EpiAxpby pe{L, lda, 1.0, 0.0};
            int npanel = 0;
            if (m2 > 0) {
                ps = GemmShape{A + (o + 2 * NB) * lda + o, lda, inv, OB, m2, NB, NB, 0};
                ps.tri = 1;
                ps.pf = 1;
                pe.C = L + (o + 2 * NB) * lda + o;
                npanel = (m2 / 32) * 2;
            }
            // XrowJob: Xt[0:o, j] = -Tt inv(L_jj)^T on 32 x 64 tiles, and one workgroup for Xt[j, j] = inv(L_jj)^T
            GemmShape xs{A, lda, inv, OB, 0, NB, NB, 0};
            EpiAxpby xse{L, lda, -1.0, 0.0};
            int nxs = 0;
            double* xdiag = nullptr;
            if (xrow) {
                if (j >= 1) {
                    xs = GemmShape{xrow->Tt, NB, inv, OB, (int)o, NB, NB, 0};
                    xs.tri = 1;      // B(k, n) = inv[n][k], zero for k > n
                    xs.pf = 1;
                    xse.C = xrow->Xt + o;
                    xse.ldc = xrow->ldx;
                    nxs = (int)(o / 32) * 2;
                }
                xdiag = xrow->Xt + o * xrow->ldx + o;
            }
            ScopedProf sp(KC_CHOL_PANEL, st);
            hipLaunchKernelGGL(chol_step_spine_kernel, dim3(36 + npanel + nxs + (xdiag ? 1 : 0)), dim3(SP_T), 0, st,
                               A + (o + NB) * lda + o, lda, inv, (int64_t)OB, L + (o + NB) * lda + o, lda, A + (o + NB) * lda + o + NB,
                               ps, pe, g_step_stamps, j, npanel, xs, xse, nxs, xdiag, xrow ? xrow->ldx : 0);
        }
    }
    if (!xrow) build_block_inverses(L, n, lda, invw, st);      // (with an XrowJob the consumers read Xt, not the 512-block inverses)
    return check_launch("emcid_cholesky_f64");
}

// Both schedules run on ONE stream.  (A look-ahead schedule on two streams — spine on the caller's, bulk on a side stream — was
// built in rounds 1-2 and lost: 13.3 -> 22.3 ms per device step inside the captured graph, every fork / join between capture
// streams costing ~70 us, and the leaf needs a whole CU's LDS, so it cannot start while the bulk GEMM keeps every CU populated;
// removed in round 5, DESIGN.md "measured and dropped".)
int cholesky_impl(double* A, double* L, int64_t dp, int64_t lda, double* invw, int* info, hipStream_t st, const ShadowJob* shadow,
                  const XrowJob* xrow) {
    if (cholesky_takes_shadow(dp)) return cholesky_fused_steps(A, L, dp, lda, invw, info, st, shadow, xrow);
    if (shadow || xrow) return fail(EMCID_ERR_BAD_ARG, "cholesky_impl", "shadow / inverse job without the fused schedule");
    return cholesky_serial(A, L, dp, lda, invw, info, st);
}

// Out[rows, n] = B (L^T)^-1 (forward) and Out = B L^-1 (backward) for a lower-triangular L [n, n], right-looking over blk-wide
// column blocks: multiply by the inverted diagonal block (block J at inv + J blk^2, leading dimension blk), then one rank-blk
// GEMM update of every remaining column.  B is consumed as scratch; n need not be a multiple of blk: the last block is the leading
// w x w part of its inverse.  The solves against a covariance factor (blk = OB) and against a session's Lp (blk = NB) both run here.
void trsm_forward(const double* L, int64_t ldl, int64_t n, int blk, const double* inv, double* B, int64_t ldb, double* Out,
                  int64_t ldo, int rows, hipStream_t st) {
    for (int64_t c = 0; c < n; c += blk) {
        const int w = (int)((n - c) < blk ? (n - c) : blk);
        GemmShape a{B + c, ldb, inv + (c / blk) * (int64_t)blk * blk, blk, rows, w, w, 0};
        a.tri = 1;   // B(k, n) = inv[n][k], zero for k > n
        {
            ScopedProf sp(KC_TRSM_DIAG, st);
            launch_gemm_f64<true, true>(a, EpiAxpby{Out + c, ldo, 1.0, 0.0}, st);
        }
        const int m = (int)(n - c - w);
        if (m > 0) {
            GemmShape b{Out + c, ldo, L + (c + w) * ldl + c, ldl, rows, m, w, 0};
            ScopedProf sp(KC_TRSM_UPDATE, st);
            launch_gemm_f64<true, true>(b, EpiAxpby{B + c + w, ldb, -1.0, 1.0}, st);
        }
    }
}

void trsm_backward(const double* L, int64_t ldl, int64_t n, int blk, const double* inv, double* B, int64_t ldb, double* Out,
                   int64_t ldo, int rows, hipStream_t st) {
    for (int64_t c = (n - 1) / blk * blk; c >= 0; c -= blk) {
        const int w = (int)((n - c) < blk ? (n - c) : blk);
        GemmShape a{B + c, ldb, inv + (c / blk) * (int64_t)blk * blk, blk, rows, w, w, 0};
        a.tri = 2;   // B(k, n) = inv[k][n], zero for k < n
        {
            ScopedProf sp(KC_TRSM_DIAG, st);
            launch_gemm_f64<true, false>(a, EpiAxpby{Out + c, ldo, 1.0, 0.0}, st);
        }
        if (c > 0) {
            GemmShape b{Out + c, ldo, L + c * ldl, ldl, rows, (int)c, w, 0};
            ScopedProf sp(KC_TRSM_UPDATE, st);
            launch_gemm_f64<true, false>(b, EpiAxpby{B, ldb, -1.0, 1.0}, st);
        }
    }
}

// Bt[M, dp] := Bt (L L^T)^-1 (Yt: scratch of the same shape), against the OB-block inverses of build_block_inverses
int cholesky_solve_impl(const double* L, int64_t dp, int64_t lda, const double* invw, double* Bt, double* Yt, int64_t Mrows,
                        int64_t ldb, hipStream_t st) {
    trsm_forward(L, lda, dp, OB, invw, Bt, ldb, Yt, ldb, (int)Mrows, st);
    trsm_backward(L, lda, dp, OB, invw, Yt, ldb, Bt, ldb, (int)Mrows, st);   // Xt written over Bt
    return check_launch("emcid_cholesky_solve_f64");
}

// X = inv(L), explicit, for `nbatch` factors at once (the dual solver's M = lam*C' factors: they do not depend on the
// concepts, so a layer's two triangular solves become two GEMMs against X).  Recursive halving over the OB-blocks:
//   inv([[L11, 0], [L21, L22]]) = [[X11, 0], [-X22 (L21 X11), X22]]
// with the diagonal OB-blocks taken from build_block_inverses.  Three quarters of the ~dp^3/3 flops sit in the two
// products of the top split (dp/2 cubed, one operand triangular: its zero part is skipped), which is what makes this
// form run at GEMM rates; a block-row recurrence has the same flops in 512-row slivers.
// T: scratch, nbatch x t_doubles >= full_inverse_scratch_doubles(dp, lda) doubles, stride s_mat.  Only the lower triangle of X
// (and the zeros inside its diagonal 128-blocks) is written; consumers never read anything else.
__global__ __launch_bounds__(256) void copy_diag_inverse_kernel(const double* __restrict__ invw, int64_t s_inv, double* __restrict__ X,
                                                                 int64_t ldx, int64_t s_x, int64_t dp) {
    const int64_t r = blockIdx.x;                 // global row
    const int64_t J = r / OB, i = r % OB;
    const int w = (int)((dp - J * OB) < OB ? (dp - J * OB) : OB);
    const double* src = invw + blockIdx.y * s_inv + J * (int64_t)OB * OB + i * OB;
    double* dst = X + blockIdx.y * s_x + r * ldx + J * OB;
    // zeros only where a diagonal 128-block could be read above the diagonal
    const int hi = (int)((i / NB + 1) * NB);
    for (int j = threadIdx.x; j < (hi < w ? hi : w); j += 256) dst[j] = (j <= i) ? src[j] : 0.0;
}

// The recursion over block ranges [b0, b1), as the list of its steps in the order they run.  When the two halves of a range are the
// same problem (equal block counts, no short last block) they are solved ONCE with the copy count doubled: `reps` copies of the
// range sit `stride` blocks apart on the diagonal and share every launch through the GEMM's second batch dimension.
struct InvStep { int b0, mid, b1, reps, stride; };
static void full_inverse_steps(int64_t dp, std::vector<InvStep>& out) {
    const int nob = (int)((dp + OB - 1) / OB);
    const bool regular = dp % OB == 0;
    std::function<void(int, int, int, int)> rec = [&](int b0, int b1, int reps, int stride) {
        const int n = b1 - b0;
        if (n <= 1) return;
        const int mid = b0 + n / 2, left = mid - b0, right = b1 - mid;
        if (regular && left == right && (reps == 1 || stride == 2 * left)) {
            rec(b0, mid, reps * 2, left);
        } else {
            rec(b0, mid, reps, stride);
            rec(mid, b1, reps, stride);
        }
        out.push_back(InvStep{b0, mid, b1, reps, stride});
    };
    rec(0, nob, 1, 0);
}

// What build_full_inverse asks of T, per factor: a step with m = r1 - rm rows below the split and nn = rm - r0 columns left of it
// writes its `reps` copies as reps * m rows of nn doubles at leading dimension lda, from T[0] on, so it reaches
// (reps * m - 1) * lda + nn doubles.  reps * m is the same at every level of a regular dp (dp / 2 rows: (dp / 2 - 1) * lda + dp / 2);
// with a short last block the top split is the largest, m = dp - 512 * (ceil(dp / 512) / 2) rows.
int64_t full_inverse_scratch_doubles(int64_t dp, int64_t lda) {
    std::vector<InvStep> steps;
    full_inverse_steps(dp, steps);
    int64_t need = 0;
    for (const InvStep& s : steps) {
        const int64_t r0 = (int64_t)s.b0 * OB, rm = (int64_t)s.mid * OB, r1 = (int64_t)s.b1 * OB < dp ? (int64_t)s.b1 * OB : dp;
        const int64_t reach = (s.reps * (r1 - rm) - 1) * lda + (rm - r0);
        if (reach > need) need = reach;
    }
    return need;
}

int build_full_inverse(const double* L, int64_t dp, int64_t lda, const double* invw, double* X, double* T, int64_t t_doubles,
                       int nbatch, int64_t s_mat, int64_t s_inv, hipStream_t st) {
    // before the first launch: a scratch that is too small would be written past its end
    const int64_t need = full_inverse_scratch_doubles(dp, lda);
    if (t_doubles < need || (nbatch > 1 && s_mat < need))
        return fail(EMCID_ERR_WORKSPACE, "build_full_inverse", "scratch T smaller than full_inverse_scratch_doubles(dp, lda)");
    ScopedProf sp(KC_INV_BUILD, st);
    hipLaunchKernelGGL(copy_diag_inverse_kernel, dim3((unsigned)dp, (unsigned)nbatch), dim3(256), 0, st, invw, s_inv, X, lda, s_mat, dp);
    // 32x64 tiles in mirrored pairs: 1.06 ms for 4 x 3072^2 vs 1.30 ms with the launcher's own choice
    // (scripts/inverse_alone.py sweeps these)
    constexpr int cfg_a = 2, cfg_b = 2, pair_ = 1;
    std::vector<InvStep> steps;
    full_inverse_steps(dp, steps);
    for (const InvStep& s : steps) {
        const int64_t r0 = (int64_t)s.b0 * OB, rm = (int64_t)s.mid * OB, r1 = (int64_t)s.b1 * OB < dp ? (int64_t)s.b1 * OB : dp;
        const int m = (int)(r1 - rm), nn = (int)(rm - r0);
        const int64_t hop = (int64_t)s.stride * OB * (lda + 1), thop = (int64_t)m * lda;      // between copies: diagonal / scratch
        GemmShape a{L + rm * lda + r0, lda, X + r0 * lda + r0, lda, m, nn, nn, 0, s_mat, s_mat, nbatch};
        a.sA2 = hop; a.sB2 = hop; a.batch2 = s.reps;
        a.tri = 2;   // B(k, n) = X11[k][n], zero for k < n
        a.pair = pair_;
        EpiAxpby ea{T, lda, 1.0, 0.0, s_mat};
        ea.sC2 = thop;
        launch_gemm_f64<true, false>(a, ea, st, cfg_a);
        GemmShape b{X + rm * lda + rm, lda, T, lda, m, nn, m, 0, s_mat, s_mat, nbatch};
        b.sA2 = hop; b.sB2 = thop; b.batch2 = s.reps;
        b.tri = 4;   // A(m, k) = X22[m][k], zero for k > m
        b.pair = pair_;
        EpiAxpby eb{X + rm * lda + r0, lda, -1.0, 0.0, s_mat};
        eb.sC2 = hop;
        launch_gemm_f64<true, false>(b, eb, st, cfg_b);
    }
    return check_launch("build_full_inverse");
}

// Both GEMMs against X contract over a triangular K range; they run as stream-K over 128x128 tiles (gemm_f64.h): the
// (tile, K-step) space cut into kStreamKWgs = 256 equal runs, whole tiles stored, the two partial tiles of a run added atomically
// into a zeroed output.  Measured for 1024 x 3072 x 3072: 218 us (zeroing included) against 253 us for mirrored 32x64
// tile pairs and 306 us for plain 64x64 tiles; 768 rows: 188 / 238 / 299 us (scripts/mb_tri.py).
//
// With the interior fast path of the small-tile ring, mirrored PAIRS of 32 x 64 tiles (every workgroup contracts over the same
// total depth, three 4-wave workgroups per compute unit, no split, no fix-up) beat the stream-K form whenever their count fills
// the chip's 768 slots evenly (scripts/mb_tri_small.py, d = 3072, us stream-K / pairs: 1024 rows 187 / 172 and 195 / 177; 768
// rows 146 / 161; 512 rows 104 / 118), and for very few rows on the backward product (128 rows: 114 / 80; 256: 98 / 81), where a
// stream-K run is mostly fix-up.
static inline bool pairs_fill_the_chip(int rows, int64_t dp, bool backward) {
    const int64_t wgs = (int64_t)((rows + 31) / 32) * (((dp + 63) / 64 + 1) / 2);
    // (at most 128 rows: the stream-K form on 64 x 64 tiles is ahead — P = Yt X of a 100-concept edit 75 -> 54 us, inv_apply 0.51 -> 0.42 ms per call)
    if (backward && rows <= 256 && rows > 128) return true;
    if (wgs <= 768) return wgs >= 614;          // one round at >= 80 % of the slots (d = 5120, 1024 rows: 640 -> 515 vs 542 us)
    const int64_t tail = wgs % 768;
    return tail == 0 || tail >= 700;
}

static inline bool few_rows_ksplit(int rows, int64_t dp) {
    static const int on = env_flag("EMCID_FEW_ROWS_KSPLIT", 1);
    return on && rows <= 128 && dp >= 1024;
}

// Yt[rows, dp] = Kt[rows, dp] * X^T  (= Kt L^-T: the forward substitution as one GEMM)
void apply_inverse_forward(const double* X, int64_t dp, const double* Kt, double* Yt, int rows, hipStream_t st, double* sk_work) {
    ScopedProf sp(KC_INV_APPLY, st);
    GemmShape g{Kt, dp, X, dp, rows, (int)dp, (int)dp, 0};
    g.tri = 1;       // B(k, n) = X[n][k], zero for k > n
    if (pairs_fill_the_chip(rows, dp, false)) {
        g.pair = 1;
        launch_gemm_f64<true, true>(g, EpiAxpby{Yt, dp, 1.0, 0.0}, st, 2);
        return;
    }
    if (few_rows_ksplit(rows, dp)) {
        // one row of 128 x 128 tiles (a 100-concept edit): 32 x 64 tiles with the contraction cut in four, partial sums added with
        // f64 atomics into a zeroed result — 36 us against 50 on the two-phase stream-K form (profiles/r06_mb_tri_small.txt)
        hipLaunchKernelGGL(zero2d_f64_kernel, dim3((unsigned)rows, 1u), dim3(256), 0, st, Yt, dp, (int64_t)0, (int)dp);
        g.ksplit = 4;
        launch_gemm_f64<true, true>(g, EpiAxpby{Yt, dp, 1.0, 1.0}, st, 2);
        return;
    }
    if (sk_work && launch_gemm_f64_streamk2<true, true>(g, EpiAxpby{Yt, dp, 1.0, 0.0}, st, kStreamKWgs, sk_work)) return;
    g.pair = 1;      // (no stream-K workspace, or more tiles than its ticket counters: mirrored tile pairs)
    launch_gemm_f64<true, true>(g, EpiAxpby{Yt, dp, 1.0, 0.0}, st, 2);
}

// C[rows, ncols] (f64, leading dimension ldc) = V[rows, dp] * X  (= V L^-1: the backward substitution as one GEMM)
void apply_inverse_backward(const double* X, int64_t dp, const double* V, int rows, int ncols, double* C, int64_t ldc,
                            hipStream_t st, double* sk_work) {
    ScopedProf sp(KC_INV_APPLY, st);
    GemmShape g{V, dp, X, dp, rows, ncols, (int)dp, 0};
    g.tri = 2;       // B(k, n) = X[k][n], zero for k < n
    if (ncols == (int)dp && pairs_fill_the_chip(rows, dp, true)) {
        g.pair = 1;
        launch_gemm_f64<true, false>(g, EpiAxpby{C, ldc, 1.0, 0.0}, st, 2);
        return;
    }
    if (ncols == (int)dp && few_rows_ksplit(rows, dp)) {
        hipLaunchKernelGGL(zero2d_f64_kernel, dim3((unsigned)rows, 1u), dim3(256), 0, st, C, ldc, (int64_t)0, ncols);
        g.ksplit = 4;
        launch_gemm_f64<true, false>(g, EpiAxpby{C, ldc, 1.0, 1.0}, st, 2);
        return;
    }
    if (sk_work && launch_gemm_f64_streamk2<true, false>(g, EpiAxpby{C, ldc, 1.0, 0.0}, st, kStreamKWgs, sk_work)) return;
    g.pair = ncols == (int)dp ? 1 : 0;      // (no stream-K workspace / too many tiles: mirrored tile pairs where the output is the whole width)
    launch_gemm_f64<true, false>(g, EpiAxpby{C, ldc, 1.0, 0.0}, st, 2);
}

// T += P P^T - Q Q^T on the lower 32 x 64 tiles in ONE launch: the contraction runs over the concatenation [P | Q] with a sign per
// K range.  The first `zpos` z-slices split P's depth, the others Q's; every slice adds its partial with f64 atomics into T,
// which the caller has set to the identity.  (Here, not with its only caller in session.hip: it inlines the GEMM tile.)
__global__ __launch_bounds__(256) void syrk_signed_kernel(GemmShape pos, GemmShape neg, EpiAxpby epi, int zpos) {
    using TA = OpTile<true, 32, 16>;
    using TB = OpTile<true, 64, 16>;
    __shared__ __attribute__((aligned(16))) double smem[2 * (TA::SIZE + TB::SIZE)];
    const bool first = (int)blockIdx.z < zpos;
    GemmShape p = first ? pos : neg;
    p.ksplit = first ? zpos : (int)gridDim.z - zpos;
    if (!first) epi.alpha = -epi.alpha;
    gemm_f64_tile<true, true, 32, 64, 16, 2, 2>(p, epi, (int)blockIdx.y, (int)blockIdx.x, first ? (int)blockIdx.z : (int)blockIdx.z - zpos, smem);
}

void assemble_schur_system(const double* Yk, int64_t ldy, int64_t dp, const double* Lkp, int64_t ldl, int64_t M, double* S, int N,
                           int Np, hipStream_t st) {
    ScopedProf sp(KC_ASSEMBLE, st);
    hipLaunchKernelGGL(eye_f64_kernel, dim3((unsigned)Np), dim3(256), 0, st, S, Np);
    GemmShape pos{Yk, ldy, Yk, ldy, N, N, (int)dp, 1};
    pos.pf = 1;
    GemmShape neg{Lkp, ldl, Lkp, ldl, N, N, (int)M, 1};
    neg.pf = M % 2 == 0 ? 1 : 0;
    auto slices = [](int64_t depth) { const int64_t z = (depth + 127) / 128; return (int)(z < 1 ? 1 : z > 8 ? 8 : z); };
    const int zpos = slices(dp), zneg = M > 0 ? slices(M) : 0;
    EpiAxpby epi{S, Np, 1.0, 1.0};
    epi.atomic = 1;
    hipLaunchKernelGGL(syrk_signed_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((N + 31) / 32), (unsigned)(zpos + zneg)), dim3(256), 0,
                       st, pos, neg, epi, zpos);
}

// ---- the library's instantiations of the fp64 GEMM launchers, and through them of the kernels (see spd_solve.h) -------------
EMCID_GEMM_F64_INSTANCES(template)

}  // namespace emcid

using namespace emcid;

extern "C" {

/* diagnostic: chol_step_leaf_kernel writes, per launch slice s < 16 and workgroup b < 512, [start, -, end, kind] (constant
 * 100 MHz clock; kind 1 leaf, 2 trailing tile, 3 shadow tile pair) at stamps_dev[(s * 512 + b) * 4], and the same for the spine
 * launches (kind 4 spine tile, 5 panel tile) at stamps_dev[((16 + s) * 512 + b) * 4]: 32 * 512 * 4 values; null switches it off.
 * Set it before the first edit of the process (captured graphs keep the pointer they were captured with). */
int emcid_debug_step_stamps(long long* stamps_dev) {
    g_step_stamps = stamps_dev;
    return EMCID_OK;
}

/* diagnostic: one leaf on a 128x128 SPD block with phase stamps (shader clock ticks) written to stamps_dev[32] */
int emcid_debug_leaf_stamps(const double* A, double* L, double* inv, int* info_dev, long long* stamps_dev, void* stream) {
    EMCID_CHECK_ARG(A && L && inv && info_dev && stamps_dev);
    hipLaunchKernelGGL(chol_leaf_kernel, dim3(1), dim3(LEAF_T), 0, (hipStream_t)stream, A, (int64_t)NB, L, (int64_t)NB, inv,
                       (int64_t)NB, info_dev, 0, stamps_dev);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int64_t emcid_inverse_workspace_doubles(int64_t dp) { return dp > 0 ? inv_doubles(round_up(dp, NB)) : 0; }

int emcid_cholesky_f64(double* A, double* L, int64_t dp, int64_t lda, double* invdiag, int* info_dev, void* stream) {
    EMCID_CHECK_ARG(A && L && invdiag && info_dev && dp > 0 && dp % NB == 0 && lda >= dp && lda % 2 == 0);
    EMCID_CHECK_ARG(aligned16(A) && aligned16(L) && aligned16(invdiag));
    return cholesky_impl(A, L, dp, lda, invdiag, info_dev, (hipStream_t)stream);
}

int emcid_cholesky_solve_f64(const double* L, int64_t dp, int64_t lda, const double* invdiag, double* Bt, double* Yt,
                             int64_t Np, int64_t ldb, void* stream) {
    EMCID_CHECK_ARG(L && invdiag && Bt && Yt && dp > 0 && dp % NB == 0 && Np > 0 && ldb >= dp && lda >= dp);
    EMCID_CHECK_ARG(aligned16(L) && aligned16(Bt) && aligned16(Yt) && lda % 2 == 0 && ldb % 2 == 0);
    return cholesky_solve_impl(L, dp, lda, invdiag, Bt, Yt, Np, ldb, (hipStream_t)stream);
}

int64_t emcid_full_inverse_scratch_doubles(int64_t dp, int64_t lda) {
    if (dp <= 0 || dp % NB != 0 || lda < dp || lda >= (int64_t)1 << 31) return -1;
    return full_inverse_scratch_doubles(dp, lda);
}

int emcid_full_inverse_f64(const double* L, int64_t dp, int64_t lda, const double* invdiag, double* X, double* scratch,
                           int64_t scratch_doubles, void* stream) {
    EMCID_CHECK_ARG(L && invdiag && X && dp > 0 && dp % NB == 0 && lda >= dp && lda % 2 == 0 && lda < (int64_t)1 << 31);
    EMCID_CHECK_ARG((scratch || scratch_doubles == 0) && scratch_doubles >= 0);
    EMCID_CHECK_ARG(aligned16(L) && aligned16(invdiag) && aligned16(X) && aligned16(scratch));
    return build_full_inverse(L, dp, lda, invdiag, X, scratch, scratch_doubles, 1, 0, 0, (hipStream_t)stream);
}

}  // extern "C"
