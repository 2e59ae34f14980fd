// Variational bottlenecks: VariationalBottleneck and AR1VariationalBottleneck
// (reference: nnx_ppo/networks/variational.py:35-81, 137-216), sequence forward and backward,
// fp32 throughout.
//
//   x [T, B, 2L] = [mean | log_std],  sigma = softplus(log_std) + min_std
//   eps = random.unit_normal(key, (L,))   z = mean + sigma * eps
//   KL  = 1/2 sum_l (mean^2 + sigma^2 - 2 ln sigma - 1)
//   l2  = mean_l (z - p~)^2,  p~ = isnan(p) ? z : p   (AR1 only; p = last z, NaN after a reset)
//   reg = kl_weight KL + ar1_weight l2
//   next key = split(key)[0]
//
// Forward: one wave per env walks the env's key chain over t in registers (every lane holds
// the same key) and the env's previous z, L / 64 elements per lane; the KL / l2 row sums are a
// fixed-order xor butterfly of the lanes' partial sums, so every lane holds the same bits and
// the result does not depend on T.  A rollout step is the same kernel at T = 1, so a row's
// bits at step t of a sequence equal those of the t-th single step.
// Backward: elementwise over [T, B, L]; the AR1 term of step t + 1 reaches z_t through the
// saved z of step t + 1 (a stencil in t, no scan, no atomics).  The forward saves eps
// (4 L bytes per row and step) so that the backward draws no noise.
//
// NaN is the reset sentinel of last_z: this file must not be built with -ffast-math
// (__builtin_isnan would fold to false).
#include "common.h"
#include "keys_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxLatent = 512;
constexpr int kPerLane = kMaxLatent / kWave;

__device__ inline float vb_softplus(float x) {
  // jax.nn.softplus = logaddexp(x, 0) = max(x, 0) + log1p(exp(-|x|))
  return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
}

__device__ inline float vb_sigma(float log_std, float min_std) {
  return vb_softplus(log_std) + min_std;
}

// random.unit_normal(key, (L,))[l] with mk = mix(key): Box-Muller from the two 24-bit halves
// of bits(key, (L,))[l].  cos(2 pi u2) as cospi(2 u2): 2 u2 is exact and cospif reduces exactly
// (no Payne-Hanek path, no scratch; see philox.h).
__device__ inline float vb_normal(uint64_t mk, int l) {
  const uint64_t b = mippo_keys::mix(mk ^ ((uint64_t)(l + 1) * mippo_keys::kM2));
  const float u1 = (float)(int64_t)((b >> 40) + 1) * (1.0f / 16777216.0f);
  const float u2 = (float)(int64_t)((b >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

struct FwdArgs {
  const float* x;         // [T, B, 2L]
  const int64_t* key0;    // [B]
  const float* last_z0;   // [B, L] or null (plain VB)
  const uint8_t* done;    // [T, B] or null
  float* z;               // [T, B, L]
  float* eps;             // [T, B, L] or null
  float* reg;             // [T, B]
  float* kl;              // [T, B] or null
  float* l2;              // [T, B] or null
  float* sigma;           // [T, B, L] or null
  int64_t* key_out;       // [B]
  float* last_z_out;      // [B, L] or null
  int64_t T, B;
  int L;
  float kl_weight, ar1_weight, min_std;
  int ar1;
};

// One step of one env row (the wave's lanes share `key`); `pz` holds the lane's previous z
// per element (NaN: no AR1 term).  Writes z / eps / sigma, returns (KL, l2) via the refs.
__device__ inline void vb_row_step(const FwdArgs& a, int64_t row, uint64_t key,
                                   float (&pz)[kPerLane], float& kl_row, float& l2_row) {
  const int lane = threadIdx.x % kWave;
  const int L = a.L;
  const float* xr = a.x + row * 2 * L;
  const uint64_t mk = mippo_keys::mix(key);
  float kl = 0.0f, l2 = 0.0f;
#pragma unroll
  for (int c = 0; c < kPerLane; ++c) {
    const int l = lane + c * kWave;
    if (l < L) {
      const float mean = xr[l];
      const float s = vb_sigma(xr[L + l], a.min_std);
      const float e = vb_normal(mk, l);
      const float zz = fmaf(s, e, mean);
      kl += ((fmaf(mean, mean, s * s) - 2.0f * logf(s)) - 1.0f);
      if (a.ar1) {
        const float p = __builtin_isnan(pz[c]) ? zz : pz[c];
        const float d = zz - p;
        l2 = fmaf(d, d, l2);
      }
      pz[c] = zz;
      const int64_t o = row * L + l;
      a.z[o] = zz;
      if (a.eps) a.eps[o] = e;
      if (a.sigma) a.sigma[o] = s;
    }
  }
  kl_row = 0.5f * wave_sum(kl);
  l2_row = a.ar1 ? wave_sum(l2) / (float)L : 0.0f;
}

__global__ void __launch_bounds__(kThreads) vb_seq_fwd_kernel(FwdArgs a) {
  const int64_t b = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  if (b >= a.B) return;  // whole waves leave together
  const int lane = threadIdx.x % kWave;
  const int L = a.L;
  const float kNaN = __builtin_nanf("");
  float pz[kPerLane];
#pragma unroll
  for (int c = 0; c < kPerLane; ++c) {
    const int l = lane + c * kWave;
    pz[c] = (a.ar1 && a.last_z0 && l < L) ? a.last_z0[b * L + l] : kNaN;
  }
  uint64_t key = (uint64_t)a.key0[b];
  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t row = t * a.B + b;
    float kl, l2;
    vb_row_step(a, row, key, pz, kl, l2);
    if (lane == 0) {
      a.reg[row] = a.ar1 ? fmaf(a.ar1_weight, l2, a.kl_weight * kl) : a.kl_weight * kl;
      if (a.kl) a.kl[row] = kl;
      if (a.l2) a.l2[row] = l2;
    }
    key = mippo_keys::mix(key + mippo_keys::kGolden);  // split(key)[0]
    if (a.done && a.done[row]) {                      // the carry resets after step t
#pragma unroll
      for (int c = 0; c < kPerLane; ++c) pz[c] = kNaN;
    }
  }
  if (lane == 0) a.key_out[b] = (int64_t)key;
  if (a.last_z_out) {
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
      const int l = lane + c * kWave;
      if (l < L) a.last_z_out[b * L + l] = pz[c];
    }
  }
}

struct BwdArgs {
  const float* x;        // [T, B, 2L]
  const float* eps;      // [T, B, L]
  const float* z;        // [T, B, L] (AR1) or null
  const float* last_z0;  // [B, L] or null
  const uint8_t* done;   // [T, B] or null
  const float* g_z;      // [T, B, L] or null (zero)
  float* g_x;            // [T, B, 2L]
  int64_t T, B;
  int L;
  float g_reg, kl_weight, ar1_weight, min_std;
  int ar1, bptt;
};

//   a_t    = g_reg ar1_w (2/L) (z_t - p_t) v_t
//   dz_t   = g_z_t + a_t - [bptt] a_{t+1}          (a_{t+1} only inside the sequence)
//   dmean  = dz_t + g_reg kl_w mean
//   dsigma = dz_t eps + g_reg kl_w (sigma - 1/sigma)
//   dlogstd = dsigma sigmoid(log_std)
__global__ void __launch_bounds__(kThreads) vb_seq_bwd_kernel(BwdArgs a) {
  const int64_t L = a.L;
  const int64_t BL = a.B * L;
  const int64_t n = a.T * BL;
  const float c_kl = a.g_reg * a.kl_weight;
  const float c_ar = a.g_reg * a.ar1_weight * (2.0f / (float)a.L);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kThreads) {
    const int64_t t = i / BL;
    const int64_t r = i - t * BL;
    const int64_t b = r / L;
    const int64_t l = r - b * L;
    const int64_t row = t * a.B + b;
    const float mean = a.x[row * 2 * L + l];
    const float ls = a.x[row * 2 * L + L + l];
    const float s = vb_sigma(ls, a.min_std);
    float dz = a.g_z ? a.g_z[i] : 0.0f;
    if (a.ar1) {
      const float zt = a.z[i];
      float p;
      if (t == 0)
        p = a.last_z0 ? a.last_z0[r] : __builtin_nanf("");
      else
        p = (a.done && a.done[row - a.B]) ? __builtin_nanf("") : a.z[i - BL];
      if (!__builtin_isnan(p)) dz += c_ar * (zt - p);
      if (a.bptt && t + 1 < a.T && !(a.done && a.done[row])) dz -= c_ar * (a.z[i + BL] - zt);
    }
    const float dmean = fmaf(c_kl, mean, dz);
    const float dsig = fmaf(dz, a.eps[i], c_kl * (s - 1.0f / s));
    const float sg = 1.0f / (1.0f + expf(-ls));
    a.g_x[row * 2 * L + l] = dmean;
    a.g_x[row * 2 * L + L + l] = dsig * sg;
  }
}

}  // namespace

extern "C" int mi_vb_max_latent(void) { return kMaxLatent; }

extern "C" int mi_vb_seq_fwd_f32(const float* x, const int64_t* key0, const float* last_z0,
                                 const uint8_t* done, float* z, float* eps, float* reg,
                                 float* kl, float* l2, float* sigma, int64_t* key_out,
                                 float* last_z_out, int64_t T, int64_t B, int64_t L,
                                 float kl_weight, float ar1_weight, float min_std, int ar1,
                                 mi_stream_t stream) {
  MI_REQUIRE(L >= 1 && L <= kMaxLatent,
             "mi_vb_seq_fwd_f32: latent size %lld outside [1, %d]", (long long)L, kMaxLatent);
  MI_REQUIRE(T >= 1 && B >= 0, "mi_vb_seq_fwd_f32: bad shape T=%lld B=%lld", (long long)T,
             (long long)B);
  if (B == 0) return 0;
  MI_REQUIRE(x && key0 && z && reg && key_out, "mi_vb_seq_fwd_f32: null pointer");
  MI_REQUIRE(ar1 || (!last_z0 && !last_z_out && !l2),
             "mi_vb_seq_fwd_f32: last_z / l2 operands belong to the AR1 form");
  FwdArgs a = {x, key0, last_z0, done, z, eps, reg, kl, l2, sigma, key_out, last_z_out,
               T, B, (int)L, kl_weight, ar1_weight, min_std, ar1 ? 1 : 0};
  const int64_t rows_per_block = kThreads / kWave;
  hipLaunchKernelGGL(vb_seq_fwd_kernel, dim3((unsigned)mippo::ceil_div(B, rows_per_block)),
                     dim3(kThreads), 0, mippo::as_stream(stream), a);
  return mippo::check_launch("mi_vb_seq_fwd_f32");
}

extern "C" int mi_vb_seq_bwd_f32(const float* x, const float* eps, const float* z,
                                 const float* last_z0, const uint8_t* done, const float* g_z,
                                 float g_reg, float* g_x, int64_t T, int64_t B, int64_t L,
                                 float kl_weight, float ar1_weight, float min_std, int ar1,
                                 int bptt, mi_stream_t stream) {
  MI_REQUIRE(L >= 1 && L <= kMaxLatent,
             "mi_vb_seq_bwd_f32: latent size %lld outside [1, %d]", (long long)L, kMaxLatent);
  MI_REQUIRE(T >= 1 && B >= 0, "mi_vb_seq_bwd_f32: bad shape T=%lld B=%lld", (long long)T,
             (long long)B);
  if (B == 0) return 0;
  MI_REQUIRE(x && eps && g_x, "mi_vb_seq_bwd_f32: null pointer");
  MI_REQUIRE(!ar1 || z, "mi_vb_seq_bwd_f32: the AR1 form needs z");
  BwdArgs a = {x, eps, z, last_z0, done, g_z, g_x, T, B, (int)L, g_reg, kl_weight,
               ar1_weight, min_std, ar1 ? 1 : 0, bptt ? 1 : 0};
  const int64_t n = T * B * L;
  const int64_t blocks = std::min<int64_t>(mippo::ceil_div(n, kThreads), mippo::kMaxStreamBlocks);
  hipLaunchKernelGGL(vb_seq_bwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0,
                     mippo::as_stream(stream), a);
  return mippo::check_launch("mi_vb_seq_bwd_f32");
}
