// psh_scattering_grad.hip -- the gradient of a row's scattering spectra with respect to the row (psh_scattering_vjp): for R
// rows of n float32 returns, J scales, G groups of rows and a cotangent cot (G x NOUT),
//   out_grad[r][t] = sum_o cot[group of r][o] d out_o(x_r) / d x_r[t],
// out_o(x_r) the row's own S1, S2, C3, C4 of psh_scattering.hip (what the row adds to its group's sum), every sample
// converted to double first, all arithmetic in double.  Host twin: shadowing_amd/scattering.py (torch.fft on the time-domain
// definition, differentiated by autograd): an independent derivation.
//
// The formulas.  All arrays over k < n / 2, psi_j real, X = F[x], Y_j = F[U_j], g_z = dL/dRe z + i dL/dIm z,
// alpha3 = cot(Re C3) + i cot(Im C3), alpha4 = cot(Re C4) + i cot(Im C4) (the cotangent of Im C4[j, j, j2] is ignored: that
// output is identically 0), a1 = cot(S1), a2 = cot(S2).  From the Fourier-domain forms of C3 and C4 (psh_scattering.hip):
//   gX[k]   = sum_{j1 <= j2} alpha3[j1,j2] Y_j1[k] psi_j2[k]^2 / n^2
//   gY_j[k] = sum_{j2 >= j} psi_j2[k]^2 / n^2 ( conj(alpha3[j,j2]) X[k] + sum_{j <= j' <= j2} alpha4[j,j',j2] Y_j'[k]
//                                              + sum_{j1 <= j} conj(alpha4[j1,j,j2]) Y_j1[k] )
// and back through the modulus, scale by scale:
//   gU_j[t] = Re sum_k gY_j[k] e^{+2 pi i k t / n} + a1[j] / n + 2 a2[j] U_j[t] / n
//   gW_j[t] = gU_j[t] W_j[t] / |W_j[t]|            (0 where W_j[t] = 0: torch's sgn; an all-zero row gets zeros, never a NaN)
//   gX[k]  += psi_j[k] F[gW_j][k] / n              (inside band j)
//   grad[t] = Re sum_k gX[k] e^{+2 pi i k t / n}.
//
// The method:
//   * One workgroup of 512 threads per row, every n-point transform in LDS, with psh_mrw_lds.h's forward transform and
//     psh_scat_lds.h's inverse.  A workgroup takes rows blockIdx.x, blockIdx.x + gridDim.x, ..; a row's gradient depends on
//     the row and its group's cot row alone and every sum below has a fixed order, so the bits do not depend on R, G, the
//     row's position or the grid.
//   * A forward sweep, j = J .. 1 (1 + 2 J transforms): F[x]; per scale the inverse of F[x] psi_j, U_j = |W_j| and its
//     forward transform Y_j, kept on k < n / 2^j (no band j2 >= j reaches further).  Y_1 is needed on k >= n / 4 by band
//     j2 = 1 alone, whose terms are formed in place while Y_1 is in the working buffer; it is kept on k < n / 4.
//   * A backward sweep, j = 1 .. J (3 J + 1 transforms): gY_j into the working buffer, zero on k >= n / 2, inverse, real
//     part; the inverse of F[x] psi_j again for W_j; gW_j; its forward transform; gX.  One inverse of gX ends the row.
//     5 J + 2 transforms against the forward's 2 J + 1.
//   * What belongs to one bin or one sample lives in the registers of the thread that owns it: thread i holds F[x][k] and
//     gX[k] for k = i, i + 512, .. (4 of each at n = 4096) and gU_j[t] for t = i, i + 512, .. (8), and every step that
//     reads or adds to them walks k or t in that order.  So F[x], gX and gU_j need neither LDS nor device memory: 48
//     registers of a thread.
//
// LDS layout (NMAX = 1024 or 4096 by n): buf, NMAX complex doubles at psh_mrw_lds.h's XOR-swizzled slots (64 KiB); keep,
// 3 NMAX / 4: Y_j of j = 2 .. J at [n / 2^j, 2 n / 2^j), Y_1 on k < n / 4 at [n / 2, 3 n / 4) (48 KiB); the group's cot row (570
// doubles at J = 10): 116.5 KiB at n = 4096, 32.5 KiB at n <= 1024.  The workspace holds one flag per workgroup (a row
// left out), which a second launch folds into out_status: no atomics of any kind.
//
// Measured on MI355X (tools/bench_scattering_generate.py: median ms of 20 calls, every case in one process, J = 9, a
// skewed-MRW ensemble made on the device; R x n = 2048 x 4096 and 32768 x 4096):
//   psh_scattering_vjp (47 R transforms of 4096 points, G = 64)        2.79     44.3
//   psh_scattering_spectra in the same run (19 R transforms)           1.50     22.6
//   ratio (the transform counts give 2.47)                             1.86     1.96
// 29 ns per transform chip-wide against the forward's 36: the forward's 210 band sums of C3 and C4 each end in a cross-lane
// reduction, the backward sweep forms gY_j bin by bin with none (the likely cause; not timed separately).  One generation
// (scattering_generate, batch 256, 200 evaluations a batch): 256 rows 2.09 s as the first call of the process, 2048 rows
// 3.68 s, 2.3 ms per evaluation of which about 0.5 ms are the two kernels by the table's time per row; sqrt(loss) 0.0189 -> 0.0011.  Kernel and torch twin
// agree within 5e-15 max_t |twin| per row (tests/test_gpu_scattering_grad.py asks for 1e-9).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_mrw_lds.h"    // mrw_slot, mrw_passes: the forward transform
#include "psh_scat_lds.h"   // scat_inverse: its counterpart

namespace psh {

namespace {

__device__ __forceinline__ double2 cadd(double2 u, double2 v) { return make_double2(u.x + v.x, u.y + v.y); }
__device__ __forceinline__ double2 cscale(double2 u, double w) { return make_double2(u.x * w, u.y * w); }
__device__ __forceinline__ double2 cconj(double2 u) { return make_double2(u.x, -u.y); }

template <int NMAX>
__global__ __launch_bounds__(PSH_SCAT_THREADS) void scatgrad_kernel(ScatGradArgs a) {
    constexpr int NT = NMAX / PSH_SCAT_THREADS;              // the samples t a thread owns
    constexpr int NK = NT / 2;                               // the bins k < n / 2 a thread owns
    __shared__ double2 buf[NMAX];
    __shared__ double2 keep[3 * NMAX / 4];
    __shared__ double cot[PSH_SCAT_MAX_NOUT];
    const int tid = (int)threadIdx.x;
    const int n = a.n, logn = a.logn, J = a.J, half = n >> 1;
    const int P3 = J * (J + 1) / 2, P4 = J * (J + 1) * (J + 2) / 6;
    const double* const c3re = cot + 2 * J;
    const double* const c3im = c3re + P3;
    const double* const c4re = c3im + P3;
    const double* const c4im = c4re + P4;
    const double inv_n = 1.0 / (double)n, inv_n2 = inv_n * inv_n;
    int excluded = 0;

    // the slot of bin k in a bit-reversed spectrum; Y_jj[k] among the kept spectra
    auto bin = [&](int k) { return mrw_slot((int)(__brev((unsigned)k) >> (32 - logn))); };
    auto kept = [&](int jj, int k) { return keep[(jj == 1 ? half : (n >> jj)) + k]; };

    for (int64_t r = (int64_t)blockIdx.x; r < a.R; r += (int64_t)gridDim.x) {
        const float* row = a.x + r * a.stride;
        double* grow = a.grad + r * a.gstride;
        const int64_t g = ((r + 1) * a.G - 1) / a.R;         // the group whose rows [floor(g R / G), floor((g+1) R / G)) hold r
        int bad = 0;
        for (int t = tid; t < n; t += PSH_SCAT_THREADS) {
            const float v = row[t];
            bad |= !isfinite(v);
            buf[mrw_slot(t)] = make_double2((double)v, 0.0);
        }
        for (int i = tid; i < a.nout; i += PSH_SCAT_THREADS) cot[i] = a.cot[g * (int64_t)a.nout + i];
        if (__syncthreads_or(bad)) {
            for (int t = tid; t < n; t += PSH_SCAT_THREADS) grow[t] = 0.0;
            excluded = 1;
            continue;
        }
        mrw_passes(buf, logn, 0);
        double2 X[NK], gX[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int k = tid + i * PSH_SCAT_THREADS;
            X[i] = k < half ? buf[bin(k)] : make_double2(0.0, 0.0);
            gX[i] = make_double2(0.0, 0.0);
        }
        __syncthreads();

        // buf[bitrev(k)] = F[x][k] psi_hat[j][k] inside band j, 0 elsewhere
        auto band_to_buf = [&](int j) {
            const int lo = n >> (j + 2), hi = n >> j;
            const double* ps = a.psi + (int64_t)(j - 1) * half;
#pragma unroll
            for (int i = 0; i < 2 * NK; ++i) {
                const int k = tid + i * PSH_SCAT_THREADS;
                if (k < n) {
                    double2 v = make_double2(0.0, 0.0);
                    if (i < NK && k > lo && k < hi) v = cscale(X[i < NK ? i : 0], ps[k]);
                    buf[bin(k)] = v;
                }
            }
        };

        // ---- the forward sweep: Y_j = F[|W_j|], kept on k < n / 2^j (Y_1 stays in buf)
        for (int j = J; j >= 1; --j) {
            band_to_buf(j);
            __syncthreads();
            scat_inverse(buf, logn);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = tid + i * PSH_SCAT_THREADS;
                if (t < n) {
                    const double2 w = buf[mrw_slot(t)];
                    buf[mrw_slot(t)] = make_double2(sqrt(w.x * w.x + w.y * w.y) * inv_n, 0.0);
                }
            }
            __syncthreads();
            mrw_passes(buf, logn, 0);
            if (j >= 2) {
                const int m = n >> j;
                for (int k = tid; k < m; k += PSH_SCAT_THREADS) keep[m + k] = buf[bin(k)];
                __syncthreads();
            }
        }

        // ---- the backward sweep
        for (int j = 1; j <= J; ++j) {
            // gY_j[k] on k < n / 2^j into buf (at j = 1 in place of Y_1[k], same thread, same slot), 0 elsewhere; what Y_j
            // adds to gX.  A bin lies in at most two bands j2.
            const int top = n >> j;
#pragma unroll
            for (int i = 0; i < 2 * NK; ++i) {
                const int k = tid + i * PSH_SCAT_THREADS;
                if (k >= n) continue;
                double2 gy = make_double2(0.0, 0.0);
                if (i < NK && k >= 1 && k < top) {
                    const double2 yj = j == 1 ? buf[bin(k)] : keep[top + k];
                    if (j == 1 && k < (n >> 2)) keep[half + k] = yj;
                    const double2 xk = X[i < NK ? i : 0];
                    double2 gx = gX[i < NK ? i : 0];
                    const int p = 31 - __clz(k);
                    const int j2a = logn - p - 2 > j ? logn - p - 2 : j, j2b = logn - p - 1 < J ? logn - p - 1 : J;
                    for (int j2 = j2a; j2 <= j2b; ++j2) {
                        if (!(k > (n >> (j2 + 2)) && k < (n >> j2))) continue;
                        const double w = a.psi[(int64_t)(j2 - 1) * half + k], w2 = w * w * inv_n2;
                        const int p3 = j2 * (j2 - 1) / 2 + (j - 1), b4 = (j2 - 1) * j2 * (j2 + 1) / 6;
                        const double2 al3 = make_double2(c3re[p3], c3im[p3]);
                        gx = cadd(gx, cscale(cmul(al3, yj), w2));
                        double2 s = cmul(cconj(al3), xk);
                        for (int jp = j; jp <= j2; ++jp) {           // C4[j, jp, j2]: the first slot
                            const int p4 = b4 + jp * (jp - 1) / 2 + (j - 1);
                            const double2 al4 = make_double2(c4re[p4], jp > j ? c4im[p4] : 0.0);
                            s = cadd(s, cmul(al4, jp == j ? yj : kept(jp, k)));
                        }
                        for (int j1 = 1; j1 <= j; ++j1) {            // C4[j1, j, j2]: the second slot
                            const int p4 = b4 + j * (j - 1) / 2 + (j1 - 1);
                            const double2 al4 = make_double2(c4re[p4], j1 < j ? -c4im[p4] : 0.0);
                            s = cadd(s, cmul(al4, j1 == j ? yj : kept(j1, k)));
                        }
                        gy = cadd(gy, cscale(s, w2));
                    }
                    gX[i < NK ? i : 0] = gx;
                }
                buf[bin(k)] = gy;
            }
            __syncthreads();
            scat_inverse(buf, logn);
            double gU[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = tid + i * PSH_SCAT_THREADS;
                gU[i] = t < n ? buf[mrw_slot(t)].x : 0.0;
            }
            __syncthreads();

            // W_j again; gW_j = gU_j W_j / |W_j|
            band_to_buf(j);
            __syncthreads();
            scat_inverse(buf, logn);
            const double b1 = cot[j - 1] * inv_n, b2 = 2.0 * cot[J + j - 1] * inv_n;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = tid + i * PSH_SCAT_THREADS;
                if (t < n) {
                    const double2 w = buf[mrw_slot(t)];
                    const double m = sqrt(w.x * w.x + w.y * w.y);
                    const double gu = gU[i] + b1 + b2 * (m * inv_n);
                    buf[mrw_slot(t)] = m > 0.0 ? make_double2(gu * (w.x / m), gu * (w.y / m)) : make_double2(0.0, 0.0);
                }
            }
            __syncthreads();
            mrw_passes(buf, logn, 0);
            {
                const int lo = n >> (j + 2), hi = n >> j;
                const double* ps = a.psi + (int64_t)(j - 1) * half;
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    const int k = tid + i * PSH_SCAT_THREADS;
                    if (k > lo && k < hi) gX[i] = cadd(gX[i], cscale(buf[bin(k)], ps[k] * inv_n));
                }
            }
            // (the next writes of buf[bitrev(k)] are by the thread that read it here)
        }

        // ---- grad = Re IDFT(gX)
#pragma unroll
        for (int i = 0; i < 2 * NK; ++i) {
            const int k = tid + i * PSH_SCAT_THREADS;
            if (k < n) buf[bin(k)] = i < NK && k < half ? gX[i < NK ? i : 0] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        scat_inverse(buf, logn);
        for (int t = tid; t < n; t += PSH_SCAT_THREADS) grow[t] = buf[mrw_slot(t)].x;
        // (the next row's samples go to the slots their thread read here; cot was last read before the barriers above)
    }
    if (tid == 0) a.flags[blockIdx.x] = excluded;
}

// the status bit: a row was left out by some workgroup
__global__ __launch_bounds__(64) void scatgrad_status_kernel(ScatGradArgs a) {
    int any = 0;
    for (int i = (int)threadIdx.x; i < a.wgs; i += 64) any |= a.flags[i];
    any = __any(any);
    if (threadIdx.x == 0) *a.status = any ? PSH_SCATTERING_STATUS_ROWS_EXCLUDED : PSH_SCATTERING_STATUS_OK;
}

}  // namespace

int scattering_grad_workgroups(int64_t R) { return (int)(R < PSH_SCATGRAD_MAX_WGS ? R : PSH_SCATGRAD_MAX_WGS); }

hipError_t launch_scattering_grad(const ScatGradArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.wgs), block(PSH_SCAT_THREADS);
    if (a.n <= 1024) hipLaunchKernelGGL((scatgrad_kernel<1024>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((scatgrad_kernel<4096>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.status) return e;
    hipLaunchKernelGGL(scatgrad_status_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
