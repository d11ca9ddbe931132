// rih_pose_opt.hip -- the update half of the pose optimiser's iteration (geo_optimizer_both_batch.py:874-880: Adam over the
// two translations and the two hands' finger quaternions, then ReduceLROnPlateau.step(loss)) for gfx950, with every scalar the
// host used to keep -- the step count, the learning rate of each parameter group, the scheduler's best loss and bad-epoch
// counter -- in one DEVICE block (rih_opt_state).  Nothing is read back, so an iteration can be captured in a hipGraph.
//   rih_adam_dev      block (chunk, tensor): 1024 elements of one table entry, 16-byte accesses where the pointers allow.
//                     It READS the state block only (learning rate, step count).
//   rih_plateau_step  one thread of one workgroup: the scheduler on the loss scalar; the only writer of the state block.
// Two launches on one stream, in that order: Adam sees the learning rate from before the scheduler saw this iteration's loss, as
// `optimizer.step(); scheduler.step(loss)` does, and no workgroup reads what another workgroup of its launch writes.
// Latency class: a few thousand elements at B <= 32.  No atomics, a fixed order: two runs are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

constexpr int OPT_TPB = 256;
constexpr int OPT_CHUNK = OPT_TPB * 4;

struct AdamDevScalars {
    float beta1, beta2, eps, step_size, inv_sqrt_bias2;
};

// torch.optim.Adam (amsgrad off, no weight decay): m += (g - m)(1 - b1); v = b2 v + (1 - b2) g^2;
// p -= (lr / bias1) * m / (sqrt(v) / sqrt(bias2) + eps).  g = m = v = 0 leaves p's bits alone (p - x * 0).
__device__ __forceinline__ void adam_dev_one(float& p, float g, float& m, float& v, bool frozen, const AdamDevScalars& a) {
    if (frozen) return;
    m += (g - m) * (1.f - a.beta1);
    v = v * a.beta2 + (1.f - a.beta2) * g * g;
    const float denom = sqrtf(v) * a.inv_sqrt_bias2 + a.eps;
    p -= a.step_size * (m / denom);
}

__device__ __forceinline__ bool frozen_at(long long i, int period, int skip) {
    return period > 0 && (int)(i % period) < skip;
}

__global__ __launch_bounds__(OPT_TPB) void adam_dev_kernel(const rih_adam_dev_entry* __restrict__ table,
                                                           const rih_opt_state* __restrict__ state, float beta1, float beta2,
                                                           float eps) {
    const rih_adam_dev_entry e = table[blockIdx.y];
    const long long n = e.n, base = (long long)blockIdx.x * OPT_CHUNK;
    if (base >= n || e.group < 0 || e.group >= RIH_OPT_MAX_GROUPS) return;        // uniform over the block
    __shared__ float corr[2];
    if (threadIdx.x == 0) {
        // bias corrections in double, as torch's Python loop computes them; step counts the iterations already done
        const double t = (double)(state->step + 1);
        const double b1 = 1.0 - pow((double)beta1, t), b2 = 1.0 - pow((double)beta2, t);
        corr[0] = (float)(state->lr[e.group] / b1);
        corr[1] = (float)(1.0 / sqrt(b2));
    }
    __syncthreads();
    AdamDevScalars a;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.step_size = corr[0]; a.inv_sqrt_bias2 = corr[1];
    const long long i = base + (long long)threadIdx.x * 4;
    if (i >= n) return;
    const bool vec = ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)e.prev) & 15) == 0);
    if (vec && i + 3 < n) {
        float4 p = *reinterpret_cast<float4*>(e.p + i);
        if (e.prev) *reinterpret_cast<float4*>(e.prev + i) = p;
        const bool f0 = frozen_at(i, e.period, e.skip), f1 = frozen_at(i + 1, e.period, e.skip),
                   f2 = frozen_at(i + 2, e.period, e.skip), f3 = frozen_at(i + 3, e.period, e.skip);
        if (f0 && f1 && f2 && f3) return;
        const float4 g = *reinterpret_cast<const float4*>(e.g + i);
        float4 m = *reinterpret_cast<float4*>(e.m + i);
        float4 v = *reinterpret_cast<float4*>(e.v + i);
        adam_dev_one(p.x, g.x, m.x, v.x, f0, a);
        adam_dev_one(p.y, g.y, m.y, v.y, f1, a);
        adam_dev_one(p.z, g.z, m.z, v.z, f2, a);
        adam_dev_one(p.w, g.w, m.w, v.w, f3, a);
        *reinterpret_cast<float4*>(e.p + i) = p;                    // a frozen lane stores the bits it loaded
        *reinterpret_cast<float4*>(e.m + i) = m;
        *reinterpret_cast<float4*>(e.v + i) = v;
    } else {
        for (long long j = i; j < n && j < i + 4; ++j) {
            if (e.prev) e.prev[j] = e.p[j];
            if (!frozen_at(j, e.period, e.skip)) adam_dev_one(e.p[j], e.g[j], e.m[j], e.v[j], false, a);
        }
    }
}

// torch.optim.lr_scheduler.ReduceLROnPlateau.step (mode 'min', threshold_mode 'rel', cooldown 0) in double, as Python runs it.
__global__ __launch_bounds__(64) void plateau_step_kernel(rih_opt_state* __restrict__ st, const float* __restrict__ loss) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double current = (double)loss[0];
    double best = st->best;
    int bad = st->num_bad_epochs;
    if (current < best * (1.0 - st->threshold)) {                   // false for a NaN loss: a bad epoch
        best = current;
        bad = 0;
    } else {
        bad += 1;
    }
    if (bad > st->patience) {
        const int ng = st->ngroups < RIH_OPT_MAX_GROUPS ? st->ngroups : RIH_OPT_MAX_GROUPS;
        for (int g = 0; g < ng; ++g) {
            const double old_lr = st->lr[g];
            const double new_lr = fmax(old_lr * st->factor, st->min_lr);
            if (old_lr - new_lr > st->eps_lr) st->lr[g] = new_lr;
        }
        bad = 0;
    }
    st->best = best;
    st->num_bad_epochs = bad;
    st->step += 1;
}

}  // namespace

extern "C" int rih_adam_dev(const rih_adam_dev_entry* table, int ntensors, int64_t max_n, const rih_opt_state* state,
                            float beta1, float beta2, float eps, void* stream) {
    if (!table || !state || ntensors < 1 || ntensors > 65535 || max_n < 1) return RIH_EINVAL;
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return RIH_EINVAL;
    const int64_t chunks = (max_n + OPT_CHUNK - 1) / OPT_CHUNK;
    if (chunks > 0x7fffffffLL) return RIH_EINVAL;
    hipLaunchKernelGGL(adam_dev_kernel, dim3((unsigned)chunks, (unsigned)ntensors), dim3(OPT_TPB), 0, (hipStream_t)stream,
                       table, state, beta1, beta2, eps);
    return (int)hipGetLastError();
}

extern "C" int rih_plateau_step(rih_opt_state* state, const float* loss, void* stream) {
    if (!state || !loss) return RIH_EINVAL;
    hipLaunchKernelGGL(plateau_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, loss);
    return (int)hipGetLastError();
}
