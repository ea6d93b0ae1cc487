// A section of sr.hip, included inside its anonymous namespace after the convergence monitor (it uses SrDt, sr_dt_psi,
// SR_NO_PK_F32, sr_mon_block_sum and SrMonState of that file): the kernels of the copy reweighting and their launches.
// sr.hip keeps the entry points and the solve loop; tests/test_gpu_sr_rw.py pins these kernels.
#pragma once

// ---- copy reweighting (include/asr_hip.h, "copy reweighting": the rule) ----------------------------------------------------------
// Three launches on a reweighting iteration, all skipping the images the monitor has stopped (stopped may be nullptr):
// energy + mass per copy, the weights per image, and the rewrite of w_eff and q per element.  The summands of the energy are
// those of sr_loss_df_dt_kernel, statement for statement; the sums follow the monitor's fixed order at the scale of one copy.
constexpr int kRwMaxCopies = ASR_RW_MAX_COPIES;

// One workgroup per copy: blockIdx.x = b * n + i.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_rw_energy_kernel(const float* __restrict__ resid, double* __restrict__ energy,
                                                                        double* __restrict__ mass, int n, int per_copy, SrDt dt,
                                                                        const int* __restrict__ stopped) {
    __shared__ double sh[4];
    const int bn = blockIdx.x;
    const int b = bn / n;
    if (stopped && stopped[b]) return;
    const float* r = resid + (int64_t)bn * per_copy;
    const float* wgt = dt.w ? dt.w + (int64_t)b * dt.w_stride + (int64_t)(bn - b * n) * per_copy : nullptr;
    double e = 0.0, a = 0.0;
    for (int p = threadIdx.x; p < per_copy; p += 256) {
        const float t = r[p];
        const float ab = fabsf(t);
        float rho;
        if (dt.loss == ASR_DF_L1) {
            rho = ab;
        } else if (dt.loss == ASR_DF_HUBER && !(ab <= dt.delta)) {
            const float lin = 2.0f * ab - dt.delta;      // 2|r| is exact
            rho = dt.delta * lin;
        } else {
            rho = t * t;
        }
        if (wgt) {
            const float u = wgt[p];
            rho = u * rho;
            a += (double)u;
        }
        e += (double)rho;
    }
    e = sr_mon_block_sum(e, sh);
    a = sr_mon_block_sum(a, sh);
    if (threadIdx.x == 0) {
        energy[bn] = e;
        mass[bn] = wgt ? a : (double)per_copy;
    }
}

// One workgroup per image; n <= kRwMaxCopies.  ebar and the active flags go through LDS; every thread ranks its copies by
// counting (n reads each) and the copy of rank (A-1)/2 publishes the scale.  hist: the row of the history, or nullptr.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_rw_weights_kernel(const double* __restrict__ energy,
                                                                         const double* __restrict__ mass, float* __restrict__ c,
                                                                         float* __restrict__ hist, double* __restrict__ scale_out,
                                                                         int n, int kind, double kappa,
                                                                         const int* __restrict__ stopped) {
    __shared__ double eb[kRwMaxCopies];
    __shared__ int act[kRwMaxCopies];
    __shared__ double scale;
    const int b = blockIdx.x;
    if (stopped && stopped[b]) return;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double a = mass[(int64_t)b * n + i];
        const double v = energy[(int64_t)b * n + i] / a;
        const bool ok = (a > 0.0) && (fabs(v) < __builtin_inf());     // false for a NaN
        eb[i] = v;
        act[i] = ok ? 1 : 0;
    }
    if (threadIdx.x == 0) scale = 0.0;
    __syncthreads();
    int A = 0;
    for (int j = 0; j < n; ++j) A += act[j];
    for (int i = threadIdx.x; i < n; i += 256) {
        if (!act[i]) continue;
        const double v = eb[i];
        int rank = 0;
        for (int j = 0; j < n; ++j)
            if (act[j] && (eb[j] < v || (eb[j] == v && j < i))) rank += 1;
        if (rank == (A - 1) / 2) scale = v;               // exactly one active copy has this rank
    }
    __syncthreads();
    const double s = scale;
    if (threadIdx.x == 0 && scale_out) scale_out[b] = s;
    const bool flat = (A == 0) || (s == 0.0);
    const double ks = kappa * s;
    for (int i = threadIdx.x; i < n; i += 256) {
        float ci = 0.0f;
        if (act[i]) {
            if (flat) {
                ci = 1.0f;
            } else {
                const double t = eb[i] / ks;
                if (kind == ASR_RW_HARD) {
                    ci = (t <= 1.0) ? 1.0f : 0.0f;
                } else {
                    const double tt = t * t;
                    const double den = 1.0 + tt;
                    ci = (float)(1.0 / den);
                }
            }
        }
        c[(int64_t)b * n + i] = ci;
        if (hist) hist[(int64_t)b * n + i] = ci;
    }
}

// One thread per element: w_eff = u * c (c itself without weights), q = w_eff * psi(r) -- the forward kernel's data-term tail.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_rw_apply_kernel(const float* __restrict__ resid, const float* __restrict__ c,
                                                                       float* __restrict__ w_eff, float* __restrict__ q_out, int n,
                                                                       int per_copy, SrDt dt, const int* __restrict__ stopped) {
    const int bn = blockIdx.x;
    const int b = bn / n;
    if (stopped && stopped[b]) return;
    const int p = blockIdx.y * 256 + threadIdx.x;
    if (p >= per_copy) return;
    const int64_t o = (int64_t)bn * per_copy + p;
    const float ci = c[bn];
    float we = ci;
    if (dt.w) we = dt.w[(int64_t)b * dt.w_stride + (int64_t)(bn - b * n) * per_copy + p] * ci;
    const float r = resid[o];
    float q = sr_dt_psi(r, dt.loss, dt.delta);
    q = we * q;
    w_eff[o] = we;
    q_out[o] = q;
}

// The objective changed at a reweighting: the stop rule of every image still running starts over (best and stall of a coupled
// group live at its first member; resetting the others' too changes nothing).
__global__ __launch_bounds__(64) SR_NO_PK_F32 void sr_rw_rearm_kernel(SrMonState s, int batch) {
    for (int b = threadIdx.x; b < batch; b += 64) {
        if (s.stopped[b]) continue;
        s.best[b] = __builtin_inf();
        s.stall[b] = 0;
    }
}

int sr_rw_energy_launch(hipStream_t s, const float* r, double* energy, double* mass, int batch, int n, int per_copy, const SrDt& dt,
                        const int* stopped) {
    hipLaunchKernelGGL(sr_rw_energy_kernel, dim3((unsigned)(batch * n)), dim3(256), 0, s, r, energy, mass, n, per_copy, dt, stopped);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
int sr_rw_weights_launch(hipStream_t s, const double* energy, const double* mass, float* c, float* hist, double* scale_out, int batch,
                         int n, int kind, double kappa, const int* stopped) {
    hipLaunchKernelGGL(sr_rw_weights_kernel, dim3((unsigned)batch), dim3(256), 0, s, energy, mass, c, hist, scale_out, n, kind, kappa,
                       stopped);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
int sr_rw_apply_launch(hipStream_t s, const float* r, const float* c, float* w_eff, float* q, int batch, int n, int per_copy,
                       const SrDt& dt, const int* stopped) {
    hipLaunchKernelGGL(sr_rw_apply_kernel, dim3((unsigned)(batch * n), (unsigned)asr_cdiv(per_copy, 256)), dim3(256), 0, s, r, c, w_eff,
                       q, n, per_copy, dt, stopped);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

int sr_rw_rearm_launch(hipStream_t s, const SrMonState& ms, int batch) {
    hipLaunchKernelGGL(sr_rw_rearm_kernel, dim3(1), dim3(64), 0, s, ms, batch);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
