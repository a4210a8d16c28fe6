// The readout of an edit score (emcid_main.EditScorer): what an edit did to the text encoder's own output, reduced on the device.
//   score_rows_kernel    per row pair (a, b) [and a target t]: the sums a relative distance, a cosine and a residual ratio are made
//                        of, optionally behind a LayerNorm of both rows — fp64 from exact conversions of the fp32 inputs
//   score_chains_kernel  per prompt: max / mean / end value of a per-node ratio over the prompt's chain of trie nodes
// Both follow add_layernorm_wave_kernel (attention.hip): one wave per row or prompt, four per workgroup, reductions by shuffles,
// no LDS, no atomics, plain vector loads and stores.
#include "common.h"

// (every product and sum below is rounded on its own: the reference is plain fp64 arithmetic)
#pragma clang fp contract(off)

namespace emcid {

constexpr int SCORE_MAX_V4 = 8;      // float4 chunks per lane: rows of up to 8 * 64 * 4 = 2048 columns

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[row][0..7] for row < rows; the row pair lives in registers (as the fp32 values it was loaded as) between the passes.
//   gamma != null: both rows LayerNormed in fp64 — two-pass mean and variance, x^ = (x - mean) rstd gamma + beta — else x^ = x:
//       0: ||a^ - b^||^2    1: ||b^||^2    2: ||a^||^2    3: a^ . b^
//   t != null, on the raw rows:
//       4: ||t - a||^2      5: ||t - b||^2   6: (a - b) . (t - b)
//   7 and every slot not asked for: 0.
// The difference a^ - b^ is never formed from the two normalised rows, whose roundings (1e-16 of |x^|) would be all of it when the
// rows agree to 1e-7: with d = a - b (exact in fp64), ca = a - mean_a, cb = b - mean_b and dm = mean(d)
//       a^ - b^ = gamma [ (d - dm) rstd_a + cb (rstd_a - rstd_b) ]
//       rstd_a - rstd_b = (var_b - var_a) / (sa sb (sa + sb)),  s = sqrt(var + eps),  var_a - var_b = mean((d - dm)(ca + cb))
// every term of which carries the relative error of its own few operations; identical rows give d = 0 in every column and with
// it an exact 0 in slots 0 and 6.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                          int64_t ldb, const float* __restrict__ t, int64_t ldt,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                          int rows, int cols, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;       // (whole waves leave: no lane of a wave that stays is missing from the shuffles)
    const int nv = cols / 4;
    const float4* pa = reinterpret_cast<const float4*>(a + row * lda);
    const float4* pb = reinterpret_cast<const float4*>(b + row * ldb);
    float4 va[SCORE_MAX_V4], vb[SCORE_MAX_V4];
#pragma unroll
    for (int i = 0; i < SCORE_MAX_V4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            va[i] = pa[c];
            vb[i] = pb[c];
        }
    }
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (gamma != nullptr) {
        double sa = 0.0, sb = 0.0, sd = 0.0;
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            if (lane + i * 64 < nv) {
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sa += ax[k];
                    sb += bx[k];
                    sd += ax[k] - bx[k];
                }
            }
        }
        const double n = (double)cols;
        const double ma = wave_sum(sa) / n, mb = wave_sum(sb) / n, dm = wave_sum(sd) / n;
        double qa = 0.0, qb = 0.0, qd = 0.0;
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            if (lane + i * 64 < nv) {
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ca = ax[k] - ma, cb = bx[k] - mb, dc = (ax[k] - bx[k]) - dm;
                    qa += ca * ca;
                    qb += cb * cb;
                    qd += dc * (ca + cb);
                }
            }
        }
        const double sda = sqrt(wave_sum(qa) / n + eps), sdb = sqrt(wave_sum(qb) / n + eps);
        const double ra = 1.0 / sda, rb = 1.0 / sdb;
        const double dr = -(wave_sum(qd) / n) / (sda * sdb * (sda + sdb));
        const float4* pg = reinterpret_cast<const float4*>(gamma);
        const float4* pe = reinterpret_cast<const float4*>(beta);
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            const int c = lane + i * 64;
            if (c < nv) {
                const float4 g4 = pg[c], e4 = pe[c];
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                const double g[4] = {g4.x, g4.y, g4.z, g4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ca = ax[k] - ma, cb = bx[k] - mb, dc = (ax[k] - bx[k]) - dm;
                    const double ah = ca * ra * g[k] + e[k], bh = cb * rb * g[k] + e[k];
                    const double dh = g[k] * (dc * ra + cb * dr);
                    s[0] += dh * dh;
                    s[1] += bh * bh;
                    s[2] += ah * ah;
                    s[3] += ah * bh;
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            if (lane + i * 64 < nv) {
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double d = ax[k] - bx[k];
                    s[0] += d * d;
                    s[1] += bx[k] * bx[k];
                    s[2] += ax[k] * ax[k];
                    s[3] += ax[k] * bx[k];
                }
            }
        }
    }
    if (t != nullptr) {
        const float4* pt = reinterpret_cast<const float4*>(t + row * ldt);
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            const int c = lane + i * 64;
            if (c < nv) {
                const float4 t4 = pt[c];
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                const double tx[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ta = tx[k] - ax[k], tb = tx[k] - bx[k];
                    s[4] += ta * ta;
                    s[5] += tb * tb;
                    s[6] += (ax[k] - bx[k]) * tb;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
        double2* o = reinterpret_cast<double2*>(out + row * 8);
        o[0] = make_double2(s[0], s[1]);
        o[1] = make_double2(s[2], s[3]);
        o[2] = make_double2(s[4], s[5]);
        o[3] = make_double2(s[6], 0.0);
    }
}

// out[p][0..3] = {max, mean, value at the end node, chain position of the max (the first one on a tie)} of
// r(u) = sqrt(node[u][0] / node[u][1]) (0 when both sums are 0) over the chain anc[e][0 .. depth[e]] of e = end_node[p].
// A lane takes positions lane and lane + 64.  An end node outside [0, U), a chain longer than 128 or than ld_anc, or a chain
// entry outside [0, U) reads nothing: the prompt's four outputs are NaN.
__global__ __launch_bounds__(256) void score_chains_kernel(const double* __restrict__ node, int64_t U, const int32_t* __restrict__ anc,
                                                            int64_t ld_anc, const int32_t* __restrict__ depth,
                                                            const int64_t* __restrict__ end_node, int B, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= B) return;
    const int64_t e = end_node[p];
    const bool e_ok = e >= 0 && e < U;
    const int n = e_ok ? depth[e] + 1 : 0;
    bool ok = e_ok && n >= 1 && n <= 128 && n <= ld_anc;
    double best = -1.0, sum = 0.0, last = 0.0;
    int best_pos = 1 << 30;
    if (ok) {
        const int32_t* chain = anc + e * ld_anc;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pos = lane + 64 * j;
            if (pos < n) {
                const int64_t u = chain[pos];
                if (u < 0 || u >= U) {
                    ok = false;
                } else {
                    const double2 v = *reinterpret_cast<const double2*>(node + u * 8);
                    const double r = (v.x == 0.0 && v.y == 0.0) ? 0.0 : sqrt(v.x / v.y);
                    sum += r;
                    if (r > best) {         // (positions ascend within a lane: an equal later value does not replace)
                        best = r;
                        best_pos = pos;
                    }
                    if (pos == n - 1) last = r;
                }
            }
        }
    }
    const int bad = __any(!ok);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        last += __shfl_xor(last, o, 64);       // (one lane holds the end value, the others 0)
        const double ob = __shfl_xor(best, o, 64);
        const int op = __shfl_xor(best_pos, o, 64);
        if (ob > best || (ob == best && op < best_pos)) {
            best = ob;
            best_pos = op;
        }
    }
    if (lane == 0) {
        double2* o = reinterpret_cast<double2*>(out + (int64_t)p * 4);
        if (bad) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            o[0] = make_double2(nan, nan);
            o[1] = make_double2(nan, nan);
        } else {
            o[0] = make_double2(best, sum / (double)n);
            o[1] = make_double2(last, (double)best_pos);
        }
    }
}

}  // namespace emcid

using namespace emcid;

extern "C" {

int emcid_score_rows_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const float* t, int64_t ldt, const float* gamma,
                         const float* beta, float eps, int64_t rows, int64_t cols, double* out, void* stream) {
    EMCID_CHECK_ARG(a && b && out && rows > 0 && rows < (1LL << 31) && cols > 0);
    EMCID_CHECK_ARG(cols % 4 == 0 && cols <= SCORE_MAX_V4 * 64 * 4);
    EMCID_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= cols && ldb >= cols && (t == nullptr || (ldt % 4 == 0 && ldt >= cols)));
    EMCID_CHECK_ARG((gamma == nullptr) == (beta == nullptr));
    EMCID_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(t) && aligned16(gamma) && aligned16(beta) && aligned16(out));
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, t, ldt,
                       gamma, beta, (double)eps, (int)rows, (int)cols, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_score_chains_f64(const double* node, int64_t U, const int32_t* anc, int64_t ld_anc, const int32_t* depth,
                           const int64_t* end_node, int64_t B, double* out, void* stream) {
    EMCID_CHECK_ARG(node && anc && depth && end_node && out && U > 0 && U < (1LL << 31) && ld_anc > 0 && B > 0 && B < (1LL << 31));
    EMCID_CHECK_ARG(aligned16(node) && aligned16(out));
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_chains_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, node, U, anc, ld_anc,
                       depth, end_node, (int)B, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

}  // extern "C"
