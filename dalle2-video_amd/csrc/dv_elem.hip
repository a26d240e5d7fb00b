// Byte-moving and small kernels of the Unet3D path (all HBM- or launch-bound):
//   layout conversion at the NCTHW module boundary, space-to-depth
//   (Downsample3D, dalle2_video.py:22-25), SiLU+PixelShuffle
//   (PixelShuffleUpsample3D, :64-78), q_sample + l2 loss (p_losses :1956,
//   :1997-2002), the p_sample posterior update (:1551-1664), the time MLPs
//   (:348-357, :755-761, ResnetBlock3D.time_mlp :150-155), AdamW and the
//   gradient norm (trainer.py:247-274).
#include "dv_common.h"

using namespace dv;

namespace {

int grid_for(long long work, int per_block = 256, int cap = 16384) {
  long long b = (work + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

bool objective_ok(int objective) {
  return objective == DV_OBJ_EPS || objective == DV_OBJ_X0 || objective == DV_OBJ_V;
}

#define GRID_STRIDE(i, n) \
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

template <typename T>
__global__ void ncthw_to_cl_kernel(const float* x, T* y, int B, int C, int T_, int HW, int cpad) {
  const long long npix = (long long)B * T_ * HW;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int t = (int)(ft % T_), b = (int)(ft / T_);
    for (int c = 0; c < cpad; ++c) {
      float v = c < C ? x[(((long long)b * C + c) * T_ + t) * HW + hw] : 0.f;
      y[p * cpad + c] = (T)v;
    }
  }
}

template <typename T>
__global__ void cl_to_ncthw_kernel(const T* y, int ld, float* x, int B, int C, int T_, int HW) {
  const long long npix = (long long)B * T_ * HW;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int t = (int)(ft % T_), b = (int)(ft / T_);
    for (int c = 0; c < C; ++c) x[(((long long)b * C + c) * T_ + t) * HW + hw] = (float)y[p * ld + c];
  }
}

// unit = (frame, low-res y, x, group of VEC high-res channels); grid y walks the
// low-res rows (f, y), grid x a row's (x, channel group) units: one 32-bit
// division per unit (a flat 64-bit index took four 64-bit divisions, each a
// ~150-instruction sequence, and left the pass VALU-bound)
// MODE 1 adds r0 / r1 (high-res, strides ldr0 / ldr1; null: none) to the output
// Rows past the grid's 65,535 go two per trip, both rows' loads ahead of
// either row's stores.
template <typename T>
struct ShufIn {
  u32x4 a[4];  // MODE 1: the low-res span; MODE 0: the four high-res pixels
  u32x4 b[4];  // MODE 1: r0 at the four high-res pixels; MODE 0: z (the low-res span)
  u32x4 c[4];  // MODE 1: r1 at the four high-res pixels
};
// NX: the extra sources (MODE 1: r0, r1; MODE 0: z), a template count so no
// load sits under a run-time branch (hipcc drained vmcnt at each such join)
template <typename T, int MODE, int NX>
__global__ __launch_bounds__(256, 2) void shuffle_kernel(const T* src, int lds, T* dst, int ldd, const T* z, int ldz,
                               const T* r0, int ldr0, const T* r1, int ldr1, int nf, int H, int W,
                               int C, int act) {
  constexpr int VEC = 16 / sizeof(T);
  const int cg = C / VEC;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * cg) return;
  const int x = t / cg, g = t - x * cg;
  const int c0 = g * VEC;
  const int rows = nf * H;
  auto hp_of = [&](int row, int i, int j) {
    const long long f = row / H;
    const int y = row - (int)f * H;
    return (f * 2 * H + 2 * y + i) * 2 * W + 2 * x + j;
  };
  auto load = [&](int row, ShufIn<T>& in) {
    const long long lp = (long long)row * W + x;  // low-res pixel
    if (MODE == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) in.a[q] = *(const u32x4*)(src + lp * lds + c0 * 4 + q * VEC);
      if constexpr (NX >= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) in.b[q] = *(const u32x4*)(r0 + hp_of(row, q >> 1, q & 1) * ldr0 + c0);
      }
      if constexpr (NX >= 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) in.c[q] = *(const u32x4*)(r1 + hp_of(row, q >> 1, q & 1) * ldr1 + c0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) in.a[q] = *(const u32x4*)(src + hp_of(row, q >> 1, q & 1) * lds + c0);
      if constexpr (NX >= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) in.b[q] = *(const u32x4*)(z + lp * ldz + c0 * 4 + q * VEC);
      }
    }
  };
  auto finish = [&](int row, const ShufIn<T>& in) {
    const long long lp = (long long)row * W + x;
    float lo[4 * VEC];  // low-res span, element (c - c0)*4 + i*2 + j
    if (MODE == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) Vec<T>::to_f(in.a[q], lo + q * VEC);
#pragma unroll
      for (int e = 0; e < 4 * VEC; ++e) lo[e] = act == DV_ACT_SILU ? silu_f(lo[e]) : lo[e];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float hv[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) hv[e] = lo[e * 4 + q];
        if constexpr (NX >= 1) {
          float rv[VEC];
          Vec<T>::to_f(in.b[q], rv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) hv[e] += rv[e];
        }
        if constexpr (NX >= 2) {
          float rv[VEC];
          Vec<T>::to_f(in.c[q], rv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) hv[e] += rv[e];
        }
        T o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (T)hv[e];
        *(u32x4*)(dst + hp_of(row, q >> 1, q & 1) * ldd + c0) = *(const u32x4*)o;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float hv[VEC];
        Vec<T>::to_f(in.a[q], hv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) lo[e * 4 + q] = hv[e];
      }
      if constexpr (NX >= 1) {  // backward of SiLU+shuffle: multiply by silu'(z)
        float zz[4 * VEC];
#pragma unroll
        for (int q = 0; q < 4; ++q) Vec<T>::to_f(in.b[q], zz + q * VEC);
#pragma unroll
        for (int e = 0; e < 4 * VEC; ++e) {
          const float sg = sigmoid_f(zz[e]);
          lo[e] *= sg * (1.f + zz[e] * (1.f - sg));
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        T o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (T)lo[q * VEC + e];
        *(u32x4*)(dst + lp * ldd + c0 * 4 + q * VEC) = *(const u32x4*)o;
      }
    }
  };
  const int gy = gridDim.y;
  int row = blockIdx.y;
  for (; row + gy < rows; row += 2 * gy) {
    ShufIn<T> in0, in1;
    load(row, in0);
    load(row + gy, in1);
    __builtin_amdgcn_sched_barrier(0);  // every load of both rows ahead of the math
    finish(row, in0);
    finish(row + gy, in1);
  }
  if (row < rows) {
    ShufIn<T> in0;
    load(row, in0);
    finish(row, in0);
  }
}

template <typename T>
__global__ void q_sample_kernel(const float* x0, const float* noise, const long long* t,
                                const float* sa, const float* s1m, T* y, int B, int C, int T_,
                                int HW, int cpad, int normalize, int nt) {
  const long long npix = (long long)B * T_ * HW;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int tt = (int)(ft % T_), b = (int)(ft / T_);
    const long long ti = t[b];
    // a timestep outside the schedule poisons the output (NaN) instead of
    // reading past the table (the reference's gather raises)
    const bool ok = ti >= 0 && ti < nt;
    const float a = ok ? sa[ti] : __builtin_nanf(""), s = ok ? s1m[ti] : __builtin_nanf("");
    for (int c = 0; c < cpad; ++c) {
      float v = 0.f;
      if (c < C) {
        const long long i = (((long long)b * C + c) * T_ + tt) * HW + hw;
        const float xs = normalize ? x0[i] * 2.f - 1.f : x0[i];
        v = a * xs + s * noise[i];
      }
      y[p * cpad + c] = (T)v;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mse_kernel(const T* pred, int ld, const float* target, int B,
                                                  int C, int T_, int HW, const float* w,
                                                  float* loss, float scale) {
  __shared__ float sh[4];
  const long long npix = (long long)B * T_ * HW;
  const long long stride = (long long)gridDim.x * blockDim.x;
  float acc = 0.f;
  // 4 pixels per trip, their loads independent of each other (few blocks: every
  // block ends in ONE atomic on the loss word, and same-word atomics serialise)
  for (long long p0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; p0 < npix; p0 += 4 * stride) {
    long long pp[4];
    long long tb[4];
    float wb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = p0 + u * stride;
      const bool live = p < npix;
      pp[u] = live ? p : p0;
      const int hw = (int)(pp[u] % HW);
      const long long ft = pp[u] / HW;
      const int tt = (int)(ft % T_), b = (int)(ft / T_);
      tb[u] = ((long long)b * C * T_ + tt) * HW + hw;  // channel 0 of this pixel in the NCTHW target
      wb[u] = live ? (w ? w[b] : 1.f) : 0.f;
    }
    for (int c = 0; c < C; ++c) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        d[u] = (float)pred[pp[u] * ld + c] - target[tb[u] + (long long)c * T_ * HW];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += wb[u] * d[u] * d[u];
    }
  }
  acc = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) atomicAdd(loss, acc * scale);
}

template <typename T>
__global__ void mse_bwd_kernel(const T* pred, int ld, const float* target, int B, int C, int T_,
                               int HW, const float* w, const float* dloss, float scale, T* dp,
                               int lddp) {
  const long long npix = (long long)B * T_ * HW;
  const float g = dloss[0] * scale;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int tt = (int)(ft % T_), b = (int)(ft / T_);
    const float wb = w ? w[b] : 1.f;
    for (int c = 0; c < C; ++c) {
      const float d = (float)pred[p * ld + c] - target[(((long long)b * C + c) * T_ + tt) * HW + hw];
      dp[p * lddp + c] = (T)(2.f * g * wb * d);
    }
  }
}

// l2 loss against the x0 / v target of p_losses (dalle2_video.py:1988-1995),
// formed per element from the NCTHW x_start and noise (no target tensor):
//   x0: target = xs            v: target = sqrt(a) noise - sqrt(1 - a) xs
// xs is what q_sample_kernel noised (2 x_start - 1 when `normalize`).  The trip
// shape, reduction order and single atomic per block are mse_kernel's; a
// timestep outside the schedule gives a NaN target and reads no table entry.
template <int OBJ>
__device__ __forceinline__ float loss_target(float xs0, float nz, int normalize, float a, float s) {
  const float xs = normalize ? xs0 * 2.f - 1.f : xs0;
  if constexpr (OBJ == DV_OBJ_V) return a * nz - s * xs;
  else return a != a ? a : xs;  // a is NaN for an out-of-schedule t
}

template <typename T, int OBJ>
__global__ __launch_bounds__(256) void diff_loss_kernel(const T* pred, int ld, const float* x0,
                                                        const float* noise, const long long* t,
                                                        const float* sa, const float* s1m, int B,
                                                        int C, int T_, int HW, int normalize, int nt,
                                                        const float* w, float* loss, float scale) {
  __shared__ float sh[4];
  const long long npix = (long long)B * T_ * HW;
  const long long stride = (long long)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (long long p0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; p0 < npix; p0 += 4 * stride) {
    long long pp[4];
    long long tb[4];
    float wb[4], ka[4], ks[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = p0 + u * stride;
      const bool live = p < npix;
      pp[u] = live ? p : p0;
      const int hw = (int)(pp[u] % HW);
      const long long ft = pp[u] / HW;
      const int tt = (int)(ft % T_), b = (int)(ft / T_);
      tb[u] = ((long long)b * C * T_ + tt) * HW + hw;  // channel 0 of this pixel in the NCTHW tensors
      wb[u] = live ? (w ? w[b] : 1.f) : 0.f;
      const long long ti = t[b];
      const bool ok = ti >= 0 && ti < nt;
      ka[u] = ok ? sa[ti] : __builtin_nanf("");
      ks[u] = ok ? s1m[ti] : __builtin_nanf("");
    }
    for (int c = 0; c < C; ++c) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = tb[u] + (long long)c * T_ * HW;
        d[u] = (float)pred[pp[u] * ld + c] - loss_target<OBJ>(x0[i], noise[i], normalize, ka[u], ks[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += wb[u] * d[u] * d[u];
    }
  }
  acc = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) atomicAdd(loss, acc * scale);
}

template <typename T, int OBJ>
__global__ void diff_loss_bwd_kernel(const T* pred, int ld, const float* x0, const float* noise,
                                     const long long* t, const float* sa, const float* s1m, int B,
                                     int C, int T_, int HW, int normalize, int nt, const float* w,
                                     const float* dloss, float scale, T* dp, int lddp) {
  const long long npix = (long long)B * T_ * HW;
  const float g = dloss[0] * scale;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int tt = (int)(ft % T_), b = (int)(ft / T_);
    const float wb = w ? w[b] : 1.f;
    const long long ti = t[b];
    const bool ok = ti >= 0 && ti < nt;
    const float ka = ok ? sa[ti] : __builtin_nanf(""), ks = ok ? s1m[ti] : __builtin_nanf("");
    for (int c = 0; c < C; ++c) {
      const long long i = (((long long)b * C + c) * T_ + tt) * HW + hw;
      const float d = (float)pred[p * ld + c] - loss_target<OBJ>(x0[i], noise[i], normalize, ka, ks);
      dp[p * lddp + c] = (T)(2.f * g * wb * d);
    }
  }
}

// ---------------------------------------------------------------------------
// dynamic thresholding (dynamic_threshold, dalle2_video.py:1531-1549):
//   s[b] = max(1, quantile(|x0_u[b]|, p))  with torch.quantile's linear
// interpolation: position p (N - 1) = k0 + frac (split on the host in f64),
// s = v[k0] + frac (v[k0 + 1] - v[k0]) over the order statistics v of the
// sample's N = C T H W magnitudes.  x0_u is recomputed from (x, pred, t,
// objective) in every pass; nothing but s[b] is written.
//
// One workgroup per sample, so nothing waits on another workgroup and the
// only state is LDS.  v[k0] is found exactly by a radix select over the bit
// patterns of the magnitudes (for non-negative floats the unsigned order of
// the patterns is the order of the values): three passes over 11 + 10 + 10
// bits, each a 2048-bin LDS histogram of the elements that match the prefix
// chosen so far, a block-wide scan of the bins, and the bin holding the
// remaining rank.  The last bin is one value; if it holds more elements than
// the remaining rank + 1, v[k0 + 1] is that value as well, otherwise a fourth
// pass takes the minimum pattern above it.  Integer counts only: the result
// does not depend on the order the atomics land in.  A magnitude that is not
// finite (or an out-of-schedule t) makes s[b] NaN.
// ---------------------------------------------------------------------------
constexpr int DT_THREADS = 1024, DT_BINS = 2048;

// (kx, kp) of x0_u = kx x - kp pred.  kp_tab == NULL: kx_tab is alphas_cumprod
// and the pair is derived as ddim_step_kernel derives it; otherwise the two
// gathered tables of p_sample_kernel.
template <int OBJ>
__device__ __forceinline__ void x0_coefs(const float* kx_tab, const float* kp_tab, long long ti,
                                         float& kx, float& kp) {
  if constexpr (OBJ == DV_OBJ_X0) {
    kx = 0.f;
    kp = -1.f;
  } else if (kp_tab) {
    kx = kx_tab[ti];
    kp = kp_tab[ti];
  } else {
    const float a = kx_tab[ti];
    if constexpr (OBJ == DV_OBJ_EPS) {
      kx = sqrtf(1.f / a);
      kp = sqrtf((1.f - a) / a);
    } else {
      kx = sqrtf(a);
      kp = sqrtf(1.f - a);
    }
  }
}

template <typename T, int OBJ>
__global__ __launch_bounds__(DT_THREADS) void dyn_thres_kernel(const float* x, const T* pred, int ld,
                                                              const long long* t, const float* kx_tab,
                                                              const float* kp_tab, int C, int T_,
                                                              int HW, int nt, long long k0,
                                                              float frac, float* s_out) {
  __shared__ unsigned hist[DT_BINS];
  __shared__ unsigned wsum[DT_THREADS / 64];
  __shared__ unsigned sel_bin, sel_rank, sel_cnt, bad, next_min;
  const int tid = threadIdx.x, b = blockIdx.x;
  const long long ti = t[b];
  if (ti < 0 || ti >= nt) {  // uniform over the workgroup
    if (tid == 0) s_out[b] = __builtin_nanf("");
    return;
  }
  float kx, kp;
  x0_coefs<OBJ>(kx_tab, kp_tab, ti, kx, kp);
  const int npix = T_ * HW;  // host: C * npix < 2^31
  const float* xb = x + (long long)b * C * npix;
  // |x0_u| of channel c at pixel q of this sample, as its bit pattern
  auto mag = [&](int q, int c) -> unsigned {
    const float xv = xb[(long long)c * npix + q];
    const float e = ld > 0 ? (float)pred[((long long)b * npix + q) * ld + c]
                           : ((const float*)pred)[((long long)b * C + c) * npix + q];
    float x0u;
    if constexpr (OBJ == DV_OBJ_X0) x0u = e;
    else x0u = kx * xv - kp * e;
    return __float_as_uint(x0u) & 0x7fffffffu;
  };
  if (tid == 0) {
    bad = 0u;
    next_min = 0xffffffffu;
  }
  unsigned prefix = 0u, prefix_mask = 0u, rank = (unsigned)k0, cnt_eq = 0u;
  constexpr int SHIFT[3] = {20, 10, 0}, NBITS[3] = {11, 10, 10};
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    for (int i = tid; i < DT_BINS; i += DT_THREADS) hist[i] = 0u;
    __syncthreads();
    const unsigned bin_mask = (1u << NBITS[pass]) - 1u;
    bool nonfinite = false;
    for (int q = tid; q < npix; q += DT_THREADS) {
      for (int c = 0; c < C; ++c) {
        const unsigned m = mag(q, c);
        nonfinite |= m >= 0x7f800000u;
        if ((m & prefix_mask) == prefix) atomicAdd(&hist[(m >> SHIFT[pass]) & bin_mask], 1u);
      }
    }
    if (pass == 0 && nonfinite) bad = 1u;  // (any writer stores the same value)
    __syncthreads();
    // inclusive scan of the bins, two per thread
    const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    unsigned incl = h0 + h1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o, 64);
      if ((tid & 63) >= o) incl += up;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned base = 0u;
    for (int w = 0; w < (tid >> 6); ++w) base += wsum[w];
    const unsigned excl = base + incl - (h0 + h1);
    if (rank >= excl && rank < excl + h0 + h1) {  // exactly one thread: the counts sum to > rank
      const bool second = rank >= excl + h0;
      sel_bin = 2 * tid + (second ? 1 : 0);
      sel_rank = rank - excl - (second ? h0 : 0u);
      sel_cnt = second ? h1 : h0;
    }
    __syncthreads();
    prefix |= sel_bin << SHIFT[pass];
    prefix_mask |= bin_mask << SHIFT[pass];
    rank = sel_rank;
    cnt_eq = sel_cnt;
    __syncthreads();  // sel_* and hist are rewritten by the next pass
  }
  // prefix is v[k0]; cnt_eq elements equal it and `rank` of them sort below k0
  unsigned hi = prefix;
  if (frac > 0.f && rank + 1 >= cnt_eq) {  // v[k0 + 1] is the next larger value (uniform branch)
    unsigned mn = 0xffffffffu;
    for (int q = tid; q < npix; q += DT_THREADS)
      for (int c = 0; c < C; ++c) {
        const unsigned m = mag(q, c);
        if (m > prefix && m < mn) mn = m;
      }
    atomicMin(&next_min, mn);
    __syncthreads();
    hi = next_min;
  }
  if (tid == 0) {
    const float v0 = __uint_as_float(prefix), v1 = __uint_as_float(hi);
    const float qv = frac > 0.f ? v0 + frac * (v1 - v0) : v0;
    s_out[b] = bad ? __builtin_nanf("") : fmaxf(qv, 1.f);
  }
}

// freqs[k] = exp(-k*ln(1e4)/(half-1)) is a constant table built once on the host
// exactly as SinusoidalPosEmb builds it; t is cast to f32 (time.type_as(x)).
__global__ void sinusoidal_kernel(const long long* t, const float* freqs, float* out, int B, int dim) {
  const int half = dim / 2;
  GRID_STRIDE(i, (long long)B * dim) {
    const int b = (int)(i / dim), k = (int)(i % dim);
    const float a = (float)t[b] * freqs[k < half ? k : k - half];
    out[i] = k < half ? sinf(a) : cosf(a);
  }
}

__device__ __forceinline__ float act_in_f(float x, int act) { return act == 1 ? silu_f(x) : x; }
__device__ __forceinline__ float act_in_d(float x, int act) {
  if (act != 1) return 1.f;
  const float s = sigmoid_f(x);
  return s * (1.f + x * (1.f - s));
}
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// y[b][n] = act_out(sum_k act_in(x[b][k]) W[n][k] + bias[n]); one wave per n
__global__ __launch_bounds__(256) void linear_small_kernel(const float* x, int ldx, const float* W,
                                                           const float* bias, float* y, int ldy,
                                                           float* z, int B, int K, int N,
                                                           int act_in, int act_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += act_in_f(x[(long long)b * ldx + k], act_in) * W[(long long)n * K + k];
    s = wave_sum(s);
    if (lane == 0) {
      s += bias ? bias[n] : 0.f;
      if (z) z[(long long)b * N + n] = s;
      y[(long long)b * ldy + n] = act_out == 2 ? gelu_f(s) : s;
    }
  }
}

__device__ __forceinline__ float lin_g(const float* dy, int lddy, const float* z, int b, int n, int N,
                                       int act_out) {
  const float d = dy[(long long)b * lddy + n];
  return act_out == 2 ? d * gelu_d(z[(long long)b * N + n]) : d;
}

__global__ void linear_small_dw_kernel(const float* dy, int lddy, const float* x, int ldx,
                                       const float* z, float* dW, float* db, int B, int K, int N,
                                       int act_in, int act_out, int accumulate) {
  GRID_STRIDE(i, (long long)N * K) {
    const int n = (int)(i / K), k = (int)(i % K);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
      const float g = lin_g(dy, lddy, z, b, n, N, act_out);
      s += g * act_in_f(x[(long long)b * ldx + k], act_in);
      sb += g;
    }
    dW[i] = accumulate ? dW[i] + s : s;
    if (db && k == 0) db[n] = accumulate ? db[n] + sb : sb;
  }
}

// dx[b][k] (+)= act_in'(x) * sum_n g[b][n] W[n][k].  Block = 256 k-columns x
// one 32-row slice of n (grid.y); g for the slice is staged in LDS once, W
// rows are streamed coalesced with 8 loads in flight; slices meet in f32
// atomics (dx pre-zeroed or accumulated into).  B <= 16.
__global__ __launch_bounds__(256) void linear_small_dx_kernel(const float* dy, int lddy,
                                                              const float* x, int ldx,
                                                              const float* W, const float* z,
                                                              float* dx, int lddx, int B, int K,
                                                              int N, int act_in, int act_out) {
  constexpr int MAXB = 16, NS = 32;
  __shared__ float gs[MAXB][NS];
  const int n0 = blockIdx.y * NS;
  const int nend = min(NS, N - n0);
  for (int i = threadIdx.x; i < MAXB * NS; i += 256) {
    const int b = i / NS, nn = i % NS;
    gs[b][nn] = (b < B && nn < nend) ? lin_g(dy, lddy, z, b, n0 + nn, N, act_out) : 0.f;
  }
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float acc[MAXB];
#pragma unroll
  for (int b = 0; b < MAXB; ++b) acc[b] = 0.f;
  const float* wp = W + (long long)n0 * K + k;
#pragma unroll 8
  for (int nn = 0; nn < nend; ++nn) {
    const float w = wp[(long long)nn * K];
#pragma unroll
    for (int b = 0; b < MAXB; ++b) acc[b] += gs[b][nn] * w;  // rows b >= B are zero
  }
  for (int b = 0; b < B; ++b)
    atomicAdd(dx + (long long)b * lddx + k, acc[b] * act_in_d(x[(long long)b * ldx + k], act_in));
}


// ---------------------------------------------------------------------------
// grouped small linears (dv_linear_group_*): every entry's rows are cut into
// 64-row workgroup tiles; the entry table rides in the kernel arguments (no
// device table, graph-capture safe).  Forward: 4 lanes per output row stream
// its W row in 16-B pieces against act_in(x) staged in LDS, then a 2-step
// lane reduction.  Backward: the same row mapping writes dW / db; for dx each
// thread owns a k column and streams the tile's W rows coalesced, and the
// tiles meet in f32 atomics in `ws`; the workgroup arriving last applies
// act_in'(x), writes dx and re-zeroes ws.
// ---------------------------------------------------------------------------
constexpr int LG_MAX = 48, LG_ROWS = 64, LG_MAXB = 8, LG_MAXK = 512;
struct LinGroupArgs {
  const float* x;
  float* dx;
  float* ws;
  int B, K, act_in, n, acc_dx, finalize;
  int blk0[LG_MAX + 1];
  DvLinEntry e[LG_MAX];
};

__device__ __forceinline__ int lg_entry(const LinGroupArgs& a, int blk) {
  int e = 0;
  while (e + 1 < a.n && blk >= a.blk0[e + 1]) ++e;
  return e;
}

// act_in(x) into LDS: every thread's (at most 16) loads issued together from
// clamped indices (a run-time trip count left one load in flight per thread)
__device__ __forceinline__ void lg_stage_x(const LinGroupArgs& a, float* xs) {
  const int nx = a.B * a.K, tid = threadIdx.x;
  float v[LG_MAXB * LG_MAXK / 256];
#pragma unroll
  for (int u = 0; u < LG_MAXB * LG_MAXK / 256; ++u) v[u] = a.x[min(tid + 256 * u, nx - 1)];
#pragma unroll
  for (int u = 0; u < LG_MAXB * LG_MAXK / 256; ++u)
    if (tid + 256 * u < nx) xs[tid + 256 * u] = act_in_f(v[u], a.act_in);
}

__global__ __launch_bounds__(256) void linear_group_fwd_kernel(LinGroupArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[LG_MAXB * LG_MAXK];
  const int tid = threadIdx.x;
  const int e = lg_entry(a, blockIdx.x);
  const DvLinEntry E = a.e[e];
  const int lane = tid & 63, q = lane & 3;
  const int n = (blockIdx.x - a.blk0[e]) * LG_ROWS + (tid >> 6) * 16 + (lane >> 2);
  // the lane's W pieces (k = 4q + 16u), 8 at a time in flight; rows past the
  // entry and k past K read clamped addresses and are masked (the loop waited
  // for each load before the next with one load per trip under a branch)
  const float* wr = E.w + (long long)min(n, E.n - 1) * a.K;
  constexpr int U = 8;
  f32x4 w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = *(const f32x4*)(wr + min(q * 4 + 16 * u, a.K - 4));
  lg_stage_x(a, xs);
  __syncthreads();
  float acc[LG_MAXB];
#pragma unroll
  for (int b = 0; b < LG_MAXB; ++b) acc[b] = 0.f;
  for (int k0 = 0; k0 < a.K; k0 += 16 * U) {
    f32x4 wn[U];
    if (k0 + 16 * U < a.K) {
#pragma unroll
      for (int u = 0; u < U; ++u) wn[u] = *(const f32x4*)(wr + min(k0 + 16 * U + q * 4 + 16 * u, a.K - 4));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + q * 4 + 16 * u;
      if (k < a.K) {
#pragma unroll
        for (int b = 0; b < LG_MAXB; ++b) {
          if (b < a.B) {
            const f32x4 xv = *(const f32x4*)(xs + b * a.K + k);
            acc[b] += w[u][0] * xv[0] + w[u][1] * xv[1] + w[u][2] * xv[2] + w[u][3] * xv[3];
          }
        }
      }
    }
    if (k0 + 16 * U < a.K) {
#pragma unroll
      for (int u = 0; u < U; ++u) w[u] = wn[u];
    }
  }
#pragma unroll
  for (int b = 0; b < LG_MAXB; ++b) {
    acc[b] += __shfl_xor(acc[b], 1, 64);
    acc[b] += __shfl_xor(acc[b], 2, 64);
  }
  if (n < E.n && q == 0) {
    const float bias = E.bias ? E.bias[n] : 0.f;
#pragma unroll
    for (int b = 0; b < LG_MAXB; ++b)
      if (b < a.B) E.y[(long long)b * E.n + n] = acc[b] + bias;
  }
}

__global__ __launch_bounds__(256) void linear_group_bwd_kernel(LinGroupArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[LG_MAXB * LG_MAXK];
  __shared__ float gs[LG_MAXB][LG_ROWS];
  __shared__ int last;
  const int tid = threadIdx.x;
  lg_stage_x(a, xs);
  const int e = lg_entry(a, blockIdx.x);
  const DvLinEntry E = a.e[e];
  const int row0 = (blockIdx.x - a.blk0[e]) * LG_ROWS;
  const int rows = min(LG_ROWS, E.n - row0);
  {
    float g[LG_MAXB * LG_ROWS / 256];
#pragma unroll
    for (int u = 0; u < LG_MAXB * LG_ROWS / 256; ++u) {
      const int i = tid + 256 * u, b = i / LG_ROWS, r = i % LG_ROWS;
      g[u] = E.y[(long long)min(b, a.B - 1) * E.n + row0 + min(r, rows - 1)];
    }
#pragma unroll
    for (int u = 0; u < LG_MAXB * LG_ROWS / 256; ++u) {
      const int i = tid + 256 * u, b = i / LG_ROWS, r = i % LG_ROWS;
      gs[b][r] = (b < a.B && r < rows) ? g[u] : 0.f;
    }
  }
  __syncthreads();
  // dW / db rows: 4 lanes per row
  if (E.dw) {
    const int lane = tid & 63, q = lane & 3, r = (tid >> 6) * 16 + (lane >> 2);
    if (r < rows) {
      const int n = row0 + r;
      float* dwr = E.dw + (long long)n * a.K;
      constexpr int U = 8;  // pieces k = k0 + 4q + 16u; the accumulated dW read U at a time
      for (int k0 = 0; k0 < a.K; k0 += 16 * U) {
        f32x4 prev[U];
        if (E.accumulate_w) {
#pragma unroll
          for (int u = 0; u < U; ++u) prev[u] = *(const f32x4*)(dwr + min(k0 + q * 4 + 16 * u, a.K - 4));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = k0 + q * 4 + 16 * u;
          if (k < a.K) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < LG_MAXB; ++b) {
              if (b < a.B) {
                const f32x4 xv = *(const f32x4*)(xs + b * a.K + k);
                s += gs[b][r] * xv;
              }
            }
            if (E.accumulate_w) s += prev[u];
            *(f32x4*)(dwr + k) = s;
          }
        }
      }
      if (E.db && q == 0) {
        float sb = 0.f;
        for (int b = 0; b < a.B; ++b) sb += gs[b][r];
        E.db[n] = E.accumulate_w ? E.db[n] + sb : sb;
      }
    }
  }
  // dx partial over this tile's rows: one thread per k column
  if (a.dx) {
    for (int k = tid; k < a.K; k += 256) {
      float acc[LG_MAXB];
#pragma unroll
      for (int b = 0; b < LG_MAXB; ++b) acc[b] = 0.f;
      const float* wp = E.w + (long long)row0 * a.K + k;
      // 8 rows per trip, their loads together (clamped rows: gs is zero past `rows`)
      for (int r0 = 0; r0 < rows; r0 += 8) {
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = wp[(long long)min(r0 + j, rows - 1) * a.K];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int b = 0; b < LG_MAXB; ++b) acc[b] += gs[b][r0 + j] * w[j];  // rows b >= B are zero
      }
      for (int b = 0; b < a.B; ++b) atomicAdd(a.ws + b * a.K + k, acc[b]);
    }
    if (!a.finalize) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's atomics are performed
    __syncthreads();
    if (tid == 0) last = atomicAdd((unsigned*)(a.ws + a.B * a.K), 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    // the last workgroup's pass is the launch's tail: every load of it in one batch
    constexpr int UF = LG_MAXB * LG_MAXK / 256;
    const int nx = a.B * a.K;
    float v[UF], xv[UF], dv[UF];
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int i = min(tid + 256 * u, nx - 1);
      v[u] = __hip_atomic_load(a.ws + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      xv[u] = a.x[i];
      dv[u] = a.acc_dx ? a.dx[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int i = tid + 256 * u;
      if (i < nx) {
        a.ws[i] = 0.f;
        a.dx[i] = dv[u] + v[u] * act_in_d(xv[u], a.act_in);
      }
    }
    if (tid == 0) *(unsigned*)(a.ws + a.B * a.K) = 0u;
  }
}

__device__ __forceinline__ void adamw_elem(float& pi, float gi, float& mi, float& vi, bool decay, float lr,
                                           float b1, float b2, float eps, float wd, float step,
                                           float bc2_sqrt) {
  if (decay) pi *= 1.f - lr * wd;
  mi = mi + (1.f - b1) * (gi - mi);
  vi = vi * b2 + (1.f - b2) * gi * gi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi = pi - step * (mi / denom);
}

// scalar form (any alignment)
__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, long long n,
                             long long n_wd, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt, const float* clip) {
  const float cc = clip ? clip[0] : 1.f;
  const float step = lr / bc1;
  GRID_STRIDE(i, n) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i] * cc, mi, vi, i < n_wd, lr, b1, b2, eps, wd, step, bc2_sqrt);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// 16-B vectors, two per thread per trip: all eight loads of a trip are issued
// before its six stores (vmcnt retires loads and stores in order, so a load
// issued behind a store would also wait for that store's write)
__global__ void adamw_vec_kernel(float* p, const float* g, float* m, float* v, long long n,
                             long long n_wd, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt, const float* clip) {
  const float cc = clip ? clip[0] : 1.f;
  const float step = lr / bc1;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  f32x4* P4 = (f32x4*)p;
  const f32x4* G4 = (const f32x4*)g;
  f32x4* M4 = (f32x4*)m;
  f32x4* V4 = (f32x4*)v;
  for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    long long ix[2] = {i0, i0 + stride};
    const bool live1 = ix[1] < n4;
    if (!live1) ix[1] = i0;  // clamped: unconditional loads, store skipped
    f32x4 pv[2], gv[2], mv[2], vv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      gv[k] = G4[ix[k]];
      pv[k] = P4[ix[k]];
      mv[k] = M4[ix[k]];
      vv[k] = V4[ix[k]];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pi = pv[k][e], mi = mv[k][e], vi = vv[k][e];
        adamw_elem(pi, gv[k][e] * cc, mi, vi, 4 * ix[k] + e < n_wd, lr, b1, b2, eps, wd, step, bc2_sqrt);
        pv[k][e] = pi;
        mv[k][e] = mi;
        vv[k][e] = vi;
      }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k == 1 && !live1) break;
      M4[ix[k]] = mv[k];
      V4[ix[k]] = vv[k];
      P4[ix[k]] = pv[k];
    }
  }
  // the n % 4 tail
  const long long t = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    float pi = p[t], mi = m[t], vi = v[t];
    adamw_elem(pi, g[t] * cc, mi, vi, t < n_wd, lr, b1, b2, eps, wd, step, bc2_sqrt);
    m[t] = mi;
    v[t] = vi;
    p[t] = pi;
  }
}

// sum of squares of the flat gradient: 16-B loads, 8 independent loads in
// flight per lane (the scalar grid-stride loop was latency-bound at ~2.7 TB/s).
// Each block writes its partial to part[blockIdx.x]; clip_coef_kernel sums
// the partials in a fixed order, so the norm — and the clipped update — is
// bit-identical run to run and on every data-parallel rank (an atomic sum
// made the ranks' weights drift apart by an ulp per step)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, long long n, float* part) {
  __shared__ float sh[4];
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
  long long n4 = 0;
  if (((uintptr_t)x & 15) == 0) {
    n4 = n / 4;
    const f32x4* x4 = (const f32x4*)x;
    long long i = t0;
    for (; i + 7 * stride < n4; i += 8 * stride) {  // 8 x 16 B in flight per lane
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = x4[i + u * stride];
      a += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      b += (v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7]);
    }
    for (; i < n4; i += stride) a += x4[i] * x4[i];
  }
  a += b;
  float acc = (a[0] + a[1]) + (a[2] + a[3]);
  for (long long i = n4 * 4 + t0; i < n; i += stride) acc += x[i] * x[i];
  acc = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// coef = prescale * min(max_norm / (||prescale * g|| + 1e-6), 1)  (prescale = 1/world
// folds the DDP average into the update; torch.nn.utils.clip_grad_norm_ semantics).
// One block: thread t sums partials t, t + 256, ... then a fixed-shape block sum.
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* part, int nparts, float max_norm,
                                                        float prescale, float* coef) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = block_sum<256>(s, sh);
  if (threadIdx.x != 0) return;
  const float norm = prescale * sqrtf(s);
  float c = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.f;
  coef[0] = prescale * (c < 1.f ? c : 1.f);
  coef[1] = norm;
}

// objective of the network output (VideoDecoder predict_x_start / predict_v)
constexpr int OBJ_EPS = DV_OBJ_EPS, OBJ_X0 = DV_OBJ_X0, OBJ_V = DV_OBJ_V;

// thresholding of the derived x0 (dynamic_threshold, dalle2_video.py:1531-1549).
// DYN = false is the eps step with the static clamp, compiled as it was before
// the objectives existed.  Every other combination runs DYN = true:
// clamp(x0, -s, s)/s with the per-sample s of dyn_thres_kernel (s >= 1; a NaN s
// poisons the sample through the division), s = 1 when dyn_s is NULL.  Static
// and dynamic thresholding of one objective are therefore the same
// instructions, and a sample whose s is 1 comes out to the bit as under the
// static clamp (x/1 is exact).
template <bool DYN>
__device__ __forceinline__ float threshold_x0(float x0, const float* dyn_s, int b) {
  if constexpr (DYN) {
    const float s = dyn_s ? dyn_s[b] : 1.f;
    return fminf(fmaxf(x0, -s), s) / s;
  } else {
    return fminf(fmaxf(x0, -1.f), 1.f);
  }
}

// x0 = kx[t] x - kp[t] pred with (kx, kp) = (sqrt(1/a), sqrt(1/a - 1)) for the
// eps objective and (sqrt(a), sqrt(1 - a)) for v (NoiseScheduler's
// predict_start_from_v); the x0 objective takes pred itself and reads neither
template <typename T, int OBJ, bool DYN>
__global__ void p_sample_kernel(const float* x, const T* eps, int ld, const float* noise,
                                const long long* t, const float* sra, const float* srm1,
                                const float* c1, const float* c2, const float* logvar,
                                const float* dyn_s, float* out, float* x0_out, int B, int C, int T_,
                                int HW, int clip, int nt) {
  const long long n = (long long)B * C * T_ * HW;
  GRID_STRIDE(i, n) {
    const int hw = (int)(i % HW);
    long long r = i / HW;
    const int tt = (int)(r % T_);
    r /= T_;
    const int c = (int)(r % C), b = (int)(r / C);
    const long long ti0 = t[b];
    const bool ok = ti0 >= 0 && ti0 < nt;  // out-of-schedule t: NaN, no OOB read
    const long long ti = ok ? ti0 : 0;
    const long long p = ((long long)b * T_ + tt) * HW + hw;
    const float e = ld > 0 ? (float)eps[p * ld + c] : ((const float*)eps)[i];
    float x0;
    if constexpr (OBJ == OBJ_X0) x0 = e;
    else x0 = sra[ti] * x[i] - srm1[ti] * e;
    if (clip) x0 = threshold_x0<DYN>(x0, dyn_s, b);
    const float mean = c1[ti] * x0 + c2[ti] * x[i];
    const float nz = ti == 0 ? 0.f : 1.f;
    out[i] = ok ? mean + nz * expf(0.5f * logvar[ti]) * noise[i] : __builtin_nanf("");
    if (x0_out) x0_out[i] = ok ? x0 : __builtin_nanf("");
  }
}

// one DDIM step t -> t_next (p_sample_loop_ddim, dalle2_video.py:1811-1876).
// The coefficients come from the two gathered alphas_cumprod entries, per
// element in f32, so one captured graph serves every step of the loop.  Each
// is written in the algebraically equal form that has no cancellation
// (a = ac[t], an = ac[t_next], a < an):
//   sqrt(1/a - 1)      = sqrt((1 - a)/a)           (1 - a is exact near a = 1)
//   1 - a/an           = (an - a)/an
//   (1 - an) - c1^2    = (1 - an) ((1 - eta^2) + eta^2 a (1 - an)/(an (1 - a)))
//   pred_noise         = eps + (x0 - clamp(x0))/sqrt(1/a - 1)
// (the literal (sqrt(1/a) x - x0)/sqrt(1/a - 1) loses ~1e-4 at t = 1).
// The other objectives give the unthresholded x0_u and the noise e_u it implies
// in the same cancellation-free way:
//   v :  x0_u = sqrt(a) x - sqrt(1 - a) v,   e_u = sqrt(1 - a) x + sqrt(a) v
//   x0:  x0_u = pred,                         e_u = (x - sqrt(a) pred)/sqrt(1 - a)
//        (its cancellation near t = 0 belongs to the objective: the network
//        output itself carries the noise only as that small difference)
//   pred_noise = e_u + (x0_u - x0)/sqrt(1/a - 1)   wherever thresholding moved x0
// t_next == 0 takes no noise and eta == 0 reads none (noise may be NULL).
template <typename T, int OBJ, bool DYN>
__global__ void ddim_step_kernel(const float* x, const T* eps, int ld, const float* noise,
                                 const long long* t, const long long* t_next, const float* ac,
                                 float eta, const float* dyn_s, float* out, float* x0_out, int B,
                                 int C, int T_, int HW, int clip, int nt) {
  const long long n = (long long)B * C * T_ * HW;
  GRID_STRIDE(i, n) {
    const int hw = (int)(i % HW);
    long long r = i / HW;
    const int tt = (int)(r % T_);
    r /= T_;
    const int c = (int)(r % C), b = (int)(r / C);
    const long long ti0 = t[b], tn0 = t_next[b];
    // out-of-schedule pair: NaN, no OOB read
    const bool ok = ti0 >= 0 && ti0 < nt && tn0 >= 0 && tn0 < ti0;
    const long long ti = ok ? ti0 : 0, tn = ok ? tn0 : 0;
    const float a = ac[ti], an = ac[tn];
    const float sra = sqrtf(1.f / a), srm1 = sqrtf((1.f - a) / a);
    const float e2 = eta * eta, om_an = 1.f - an;
    const float c1 = eta * sqrtf((an - a) / an * om_an / (1.f - a));
    const float c2 = sqrtf(om_an * ((1.f - e2) + e2 * (a * om_an / (an * (1.f - a)))));
    const long long p = ((long long)b * T_ + tt) * HW + hw;
    const float e = ld > 0 ? (float)eps[p * ld + c] : ((const float*)eps)[i];
    float x0u, eu;
    if constexpr (OBJ == OBJ_EPS) {
      x0u = sra * x[i] - srm1 * e;
      eu = e;
    } else if constexpr (OBJ == OBJ_V) {
      const float sa = sqrtf(a), s1m = sqrtf(1.f - a);
      x0u = sa * x[i] - s1m * e;
      eu = s1m * x[i] + sa * e;
    } else {
      x0u = e;
      eu = (x[i] - sqrtf(a) * e) / sqrtf(1.f - a);
    }
    const float x0 = clip ? threshold_x0<DYN>(x0u, dyn_s, b) : x0u;
    const float pn = x0 != x0u ? eu + (x0u - x0) / srm1 : eu;
    const float z = (eta != 0.f && tn != 0) ? noise[i] : 0.f;
    out[i] = ok ? x0 * sqrtf(an) + c1 * z + c2 * pn : __builtin_nanf("");
    if (x0_out) x0_out[i] = ok ? x0 : __builtin_nanf("");
  }
}

// RePaint bookkeeping of one sampling pass on the NCTHW f32 loop state, in
// place (p_sample_loop_ddim, dalle2_video.py:1822-1828, 1878-1886).  With
// k = the known clip (2 known - 1 when normalize), a = sqrt_ac, s = sqrt_1m_ac:
//   masked,   FINAL     : x = k
//   masked,   otherwise : x = a[t] k + s[t] noise                  (q_sample at t)
//   unmasked, t_from    : x = (a[t]/a[u]) x + ((s[t] a[u] - s[u] a[t])/a[u]) noise,
//                         u = t_from[b]      (NoiseScheduler.q_sample_from_to u -> t)
//   unmasked, otherwise : x is not written
// The renoise factors come from the four f32 table entries in double and are
// rounded to f32 once: s[t] a[u] - s[u] a[t] cancels (to ~1e-3 of its terms
// between neighbouring steps), which f32 products would turn into ~1e-5 of the
// factor.  A sample whose t (or, with t_from, whose t_from) is out of schedule
// has every element this call writes set to NaN; the tables are then read at 0.
struct BlendCoef {
  float ka, kn;  // masked:   ka k + kn noise
  float ua, un;  // unmasked: ua x + un noise (t_from only)
  bool ok;
};
template <bool FINAL>
__device__ __forceinline__ BlendCoef blend_coef(int b, const long long* t, const long long* t_from,
                                                const float* sa, const float* s1m, int nt) {
  BlendCoef c{1.f, 0.f, 1.f, 0.f, true};
  if constexpr (!FINAL) {
    const long long t0 = t[b], u0 = t_from ? t_from[b] : 0;
    c.ok = t0 >= 0 && t0 < nt && (!t_from || (u0 >= 0 && u0 < t0));
    const long long ti = c.ok ? t0 : 0, ui = c.ok ? u0 : 0;
    c.ka = sa[ti];
    c.kn = s1m[ti];
    if (t_from) {
      const double at = sa[ti], au = sa[ui], st = s1m[ti], su = s1m[ui];
      c.ua = (float)(at / au);
      c.un = (float)((st * au - su * at) / au);
    }
  }
  return c;
}
template <bool FINAL>
__device__ __forceinline__ float blend_one(float x, float known, float nz, bool masked, bool renoise,
                                           const BlendCoef& c, int normalize) {
  float r = x;
  if (masked) {
    const float k = normalize ? 2.f * known - 1.f : known;
    r = FINAL ? k : c.ka * k + c.kn * nz;
  } else if (renoise) {
    r = c.ua * x + c.un * nz;
  }
  return (c.ok || !(masked || renoise)) ? r : __builtin_nanf("");
}

// VEC: HW % 4 == 0 and every pointer aligned, so one thread owns four
// neighbouring pixels of one frame of one channel: float4 accesses, and the
// four mask bytes as one 32-bit word.  Otherwise one element per thread.
template <bool VEC, bool FINAL>
__global__ void inpaint_blend_kernel(float* x, const float* known, const unsigned char* mask,
                                     const float* noise, const long long* t, const long long* t_from,
                                     const float* sa, const float* s1m, int B, int C, int T_, int HW,
                                     int normalize, int nt) {
  const bool renoise = !FINAL && t_from != nullptr;
  constexpr int V = VEC ? 4 : 1;
  const int HWV = HW / V;
  const long long n = (long long)B * C * T_ * HWV;
  // the factors depend on the sample only: a thread forms them (two f64
  // divisions with t_from) when its stride enters another sample, not per trip
  int cb = -1;
  BlendCoef c{1.f, 0.f, 1.f, 0.f, true};
  GRID_STRIDE(i, n) {
    const int hw = (int)(i % HWV);
    long long r = i / HWV;
    const int tt = (int)(r % T_);
    r /= T_;
    const int b = (int)(r / C);
    const long long mi = ((long long)b * T_ + tt) * HWV + hw;
    if constexpr (VEC) {
      const unsigned m = reinterpret_cast<const unsigned*>(mask)[mi];
      if (m == 0u && !renoise) continue;
      if (b != cb) {
        c = blend_coef<FINAL>(b, t, t_from, sa, s1m, nt);
        cb = b;
      }
      float4 xv = reinterpret_cast<const float4*>(x)[i];
      const float4 kv = reinterpret_cast<const float4*>(known)[i];
      float4 nv = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (!FINAL) nv = reinterpret_cast<const float4*>(noise)[i];
      xv.x = blend_one<FINAL>(xv.x, kv.x, nv.x, (m & 0xffu) != 0, renoise, c, normalize);
      xv.y = blend_one<FINAL>(xv.y, kv.y, nv.y, (m & 0xff00u) != 0, renoise, c, normalize);
      xv.z = blend_one<FINAL>(xv.z, kv.z, nv.z, (m & 0xff0000u) != 0, renoise, c, normalize);
      xv.w = blend_one<FINAL>(xv.w, kv.w, nv.w, (m & 0xff000000u) != 0, renoise, c, normalize);
      reinterpret_cast<float4*>(x)[i] = xv;
    } else {
      const bool masked = mask[mi] != 0;
      if (!masked && !renoise) continue;
      if (b != cb) {
        c = blend_coef<FINAL>(b, t, t_from, sa, s1m, nt);
        cb = b;
      }
      const float nz = FINAL ? 0.f : noise[i];
      x[i] = blend_one<FINAL>(x[i], known[i], nz, masked, renoise, c, normalize);
    }
  }
}

// per-frame nearest resize of NCTHW f32 planes (F.interpolate(mode="nearest"),
// resize_image_to at dalle2_video.py:2257, 1129-1146); optional clamp
__device__ __forceinline__ int nearest_src(int o, int in, int out) {
  if (out == in) return o;
  if (out == 2 * in) return o >> 1;
  const float scale = (float)in / (float)out;
  const int s = (int)floorf((float)o * scale);
  return s < in - 1 ? s : in - 1;
}
__global__ void resize_nearest_kernel(const float* x, float* y, long long planes, int hin, int win,
                                      int hout, int wout, int do_clamp, float lo, float hi) {
  const long long n = planes * hout * wout;
  GRID_STRIDE(i, n) {
    const int ox = (int)(i % wout);
    const long long r = i / wout;
    const int oy = (int)(r % hout);
    const long long pl = r / hout;
    float v = x[(pl * hin + nearest_src(oy, hin, hout)) * win + nearest_src(ox, win, wout)];
    if (do_clamp) v = fminf(fmaxf(v, lo), hi);
    y[i] = v;
  }
}

// kornia gaussian_blur2d per frame: separable normalized gaussian, 'reflect' border
__device__ __forceinline__ int reflect_idx(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}
__global__ void blur_kernel(const float* x, float* y, long long planes, int H, int W, int ks,
                            const float* w1) {
  const long long n = planes * H * W;
  const int r = ks / 2;
  GRID_STRIDE(i, n) {
    const int ox = (int)(i % W);
    const long long rr = i / W;
    const int oy = (int)(rr % H);
    const long long pl = rr / H;
    float acc = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const int yy = reflect_idx(oy + dy, H);
      float row = 0.f;
      for (int dx = -r; dx <= r; ++dx) row += w1[dx + r] * x[(pl * H + yy) * W + reflect_idx(ox + dx, W)];
      acc += w1[dy + r] * row;
    }
    y[i] = acc;
  }
}

// ---- self-conditioning (Unet3D(self_cond=True), dalle2_video.py:738-745,
// 1969-1983): the first pass's prediction rides as extra input channels of
// the training input.  One thread owns a pixel, so a channels-last row is
// written once, with 16-byte stores.

// element c of pixel p of a channels-last source (f32 or bf16); NULL: zero
__device__ __forceinline__ float sc_load(const void* sc, int ldsc, int sc_bf16, long long p, int c) {
  if (!sc) return 0.f;
  return sc_bf16 ? (float)((const bf16*)sc)[p * ldsc + c] : ((const float*)sc)[p * ldsc + c];
}

// eight consecutive channels of a row, 16-byte stores (dst is 16-byte aligned:
// the row stride is a multiple of 8 elements)
__device__ __forceinline__ void store_row8(float* dst, const float* v) {
  f32x4 lo, hi;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = v[j];
    hi[j] = v[4 + j];
  }
  *(f32x4*)dst = lo;
  *(f32x4*)(dst + 4) = hi;
}
__device__ __forceinline__ void store_row8(bf16* dst, const float* v) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)v[j];  // round to nearest even
  *(bf16x8*)dst = r;
}

// q_sample_kernel with Csc self-conditioning channels after the C noised ones
template <typename T>
__global__ void q_sample_sc_kernel(const float* x0, const float* noise, const long long* t,
                                   const float* sa, const float* s1m, const void* sc, int ldsc,
                                   int sc_bf16, T* y, int B, int C, int Csc, int T_, int HW, int cpad,
                                   int normalize, int nt) {
  const long long npix = (long long)B * T_ * HW;
  GRID_STRIDE(p, npix) {
    const int hw = (int)(p % HW);
    const long long ft = p / HW;
    const int tt = (int)(ft % T_), b = (int)(ft / T_);
    const long long ti = t[b];
    const bool ok = ti >= 0 && ti < nt;  // as q_sample_kernel: NaN, no read past the table
    const float a = ok ? sa[ti] : __builtin_nanf(""), s = ok ? s1m[ti] : __builtin_nanf("");
    for (int c0 = 0; c0 < cpad; c0 += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        v[j] = 0.f;
        if (c < C) {
          const long long i = (((long long)b * C + c) * T_ + tt) * HW + hw;
          const float xs = normalize ? x0[i] * 2.f - 1.f : x0[i];
          v[j] = a * xs + s * noise[i];
        } else if (c < C + Csc) {
          v[j] = sc_load(sc, ldsc, sc_bf16, p, c - C);
        }
      }
      store_row8(y + p * cpad + c0, v);
    }
  }
}

}  // namespace

#define DISPATCH(dtype, KERNEL_CALL_F32, KERNEL_CALL_BF16) \
  do {                                                      \
    if ((dtype) == DV_F32) { KERNEL_CALL_F32; }             \
    else if ((dtype) == DV_BF16) { KERNEL_CALL_BF16; }      \
    else DV_REQUIRE(false, "unknown dtype");                \
  } while (0)

extern "C" int dv_ncthw_to_cl(int dtype, const float* x, void* y, int B, int C, int T, int H,
                              int W, int cpad, void* stream) {
  DV_REQUIRE(x && y && cpad >= C, "bad arguments");
  const long long npix = (long long)B * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (ncthw_to_cl_kernel<float><<<grid_for(npix), 256, 0, st>>>(x, (float*)y, B, C, T, H * W, cpad)),
           (ncthw_to_cl_kernel<bf16><<<grid_for(npix), 256, 0, st>>>(x, (bf16*)y, B, C, T, H * W, cpad)));
  return check_launch("ncthw_to_cl");
}

extern "C" int dv_cl_to_ncthw(int dtype, const void* y, int ld, float* x, int B, int C, int T, int H,
                              int W, void* stream) {
  DV_REQUIRE(x && y && ld >= C, "bad arguments");
  const long long npix = (long long)B * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (cl_to_ncthw_kernel<float><<<grid_for(npix), 256, 0, st>>>((const float*)y, ld, x, B, C, T, H * W)),
           (cl_to_ncthw_kernel<bf16><<<grid_for(npix), 256, 0, st>>>((const bf16*)y, ld, x, B, C, T, H * W)));
  return check_launch("cl_to_ncthw");
}

extern "C" int dv_shuffle(int dtype, int mode, const void* src, int lds, void* dst, int ldd,
                          const void* z, int ldz, const void* r0, int ldr0, const void* r1,
                          int ldr1, int nf, int H, int W, int C, int act, void* stream) {
  DV_REQUIRE(src && dst && (mode == 0 || mode == 1), "bad arguments");
  DV_REQUIRE(mode == 1 || (!r0 && !r1), "residuals are added by mode 1 only");
  if (!r0 && r1) {
    r0 = r1; ldr0 = ldr1; r1 = nullptr;
  }
  const int VEC = dtype == DV_BF16 ? 8 : 4;
  DV_REQUIRE(C % VEC == 0 && lds % VEC == 0 && ldd % VEC == 0 && (!z || ldz % VEC == 0) &&
                 (!r0 || (ldr0 % VEC == 0 && ldr0 >= C)) && (!r1 || (ldr1 % VEC == 0 && ldr1 >= C)),
             "channels / strides must be multiples of 16 bytes");
  if ((long long)nf * H * W * C == 0) return DV_OK;
  DV_REQUIRE((long long)W * (C / VEC) < (1ll << 31) && (long long)nf * H < (1ll << 31), "shape too large");
  // (a grid of fewer rows -- several row pairs per workgroup -- measured equal:
  // profiles/r05ag_shuffle_ab.txt)
  const dim3 grid((unsigned)((W * (C / VEC) + 255) / 256), (unsigned)std::min(nf * H, 65535));
  hipStream_t st = (hipStream_t)stream;
  const int nx = mode == 0 ? (z ? 1 : 0) : (r1 ? 2 : r0 ? 1 : 0);
#define DV_SH(TT, M, NX) shuffle_kernel<TT, M, NX><<<grid, 256, 0, st>>>((const TT*)src, lds, (TT*)dst, ldd, \
    (const TT*)z, ldz, (const TT*)r0, ldr0, (const TT*)r1, ldr1, nf, H, W, C, act)
#define DV_SH_T(TT)                          \
  if (mode == 0) {                           \
    if (nx) DV_SH(TT, 0, 1);                 \
    else DV_SH(TT, 0, 0);                    \
  } else {                                   \
    if (nx == 2) DV_SH(TT, 1, 2);            \
    else if (nx == 1) DV_SH(TT, 1, 1);       \
    else DV_SH(TT, 1, 0);                    \
  }
  if (dtype == DV_F32) {
    DV_SH_T(float)
  } else {
    DV_SH_T(bf16)
  }
#undef DV_SH_T
#undef DV_SH
  return check_launch("shuffle");
}

extern "C" int dv_q_sample(int dtype, const float* x0, const float* noise, const long long* t,
                           const float* sqrt_ac, const float* sqrt_1m_ac, void* y, int B, int C,
                           int T, int H, int W, int cpad, int normalize, int num_timesteps,
                           void* stream) {
  DV_REQUIRE(x0 && noise && t && sqrt_ac && sqrt_1m_ac && y && cpad >= C && num_timesteps > 0,
             "bad arguments");
  const long long npix = (long long)B * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (q_sample_kernel<float><<<grid_for(npix), 256, 0, st>>>(x0, noise, t, sqrt_ac, sqrt_1m_ac, (float*)y, B, C, T, H * W, cpad, normalize, num_timesteps)),
           (q_sample_kernel<bf16><<<grid_for(npix), 256, 0, st>>>(x0, noise, t, sqrt_ac, sqrt_1m_ac, (bf16*)y, B, C, T, H * W, cpad, normalize, num_timesteps)));
  return check_launch("q_sample");
}

extern "C" int dv_mse_loss(int dtype, const void* pred, int ld, const float* target, int B, int C,
                           int T, int H, int W, const float* sample_w, float* loss, void* stream) {
  DV_REQUIRE(pred && target && loss, "bad arguments");
  const long long npix = (long long)B * T * H * W;
  const float scale = 1.f / (float)((double)B * C * T * H * W);
  hipStream_t st = (hipStream_t)stream;
  zero_f32(loss, 1, st);
  const int g = grid_for((npix + 3) / 4, 256, 256);
  DISPATCH(dtype,
           (mse_kernel<float><<<g, 256, 0, st>>>((const float*)pred, ld, target, B, C, T, H * W, sample_w, loss, scale)),
           (mse_kernel<bf16><<<g, 256, 0, st>>>((const bf16*)pred, ld, target, B, C, T, H * W, sample_w, loss, scale)));
  return check_launch("mse_loss");
}

extern "C" int dv_mse_loss_bwd(int dtype, const void* pred, int ld, const float* target, int B,
                               int C, int T, int H, int W, const float* sample_w,
                               const float* dloss, void* dpred, int lddp, void* stream) {
  DV_REQUIRE(pred && target && dloss && dpred, "bad arguments");
  const long long npix = (long long)B * T * H * W;
  const float scale = 1.f / (float)((double)B * C * T * H * W);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (mse_bwd_kernel<float><<<grid_for(npix), 256, 0, st>>>((const float*)pred, ld, target, B, C, T, H * W, sample_w, dloss, scale, (float*)dpred, lddp)),
           (mse_bwd_kernel<bf16><<<grid_for(npix), 256, 0, st>>>((const bf16*)pred, ld, target, B, C, T, H * W, sample_w, dloss, scale, (bf16*)dpred, lddp)));
  return check_launch("mse_loss_bwd");
}

extern "C" int dv_diffusion_loss(int dtype, const void* pred, int ld, const float* x_start,
                                 const float* noise, const long long* t, const float* sqrt_ac,
                                 const float* sqrt_1m_ac, int B, int C, int T, int H, int W,
                                 int normalize, int objective, int num_timesteps,
                                 const float* sample_w, float* loss, void* stream) {
  DV_REQUIRE(pred && x_start && noise && t && sqrt_ac && sqrt_1m_ac && loss && num_timesteps > 0,
             "bad arguments");
  DV_REQUIRE(objective_ok(objective), "objective is DV_OBJ_EPS, DV_OBJ_X0 or DV_OBJ_V");
  // the eps target is the noise tensor as it stands: the plain l2 kernel
  if (objective == DV_OBJ_EPS) return dv_mse_loss(dtype, pred, ld, noise, B, C, T, H, W, sample_w, loss, stream);
  DV_REQUIRE(dtype == DV_F32 || dtype == DV_BF16, "unknown dtype");
  const long long npix = (long long)B * T * H * W;
  const float scale = 1.f / (float)((double)B * C * T * H * W);
  hipStream_t st = (hipStream_t)stream;
  zero_f32(loss, 1, st);
  const int g = grid_for((npix + 3) / 4, 256, 256);
#define DV_DL(TT, OBJ) diff_loss_kernel<TT, OBJ><<<g, 256, 0, st>>>((const TT*)pred, ld, x_start, noise, t, \
    sqrt_ac, sqrt_1m_ac, B, C, T, H * W, normalize, num_timesteps, sample_w, loss, scale)
  if (objective == DV_OBJ_X0) {
    if (dtype == DV_F32) DV_DL(float, DV_OBJ_X0); else DV_DL(bf16, DV_OBJ_X0);
  } else {
    if (dtype == DV_F32) DV_DL(float, DV_OBJ_V); else DV_DL(bf16, DV_OBJ_V);
  }
#undef DV_DL
  return check_launch("diffusion_loss");
}

extern "C" int dv_diffusion_loss_bwd(int dtype, const void* pred, int ld, const float* x_start,
                                     const float* noise, const long long* t, const float* sqrt_ac,
                                     const float* sqrt_1m_ac, int B, int C, int T, int H, int W,
                                     int normalize, int objective, int num_timesteps,
                                     const float* sample_w, const float* dloss, void* dpred,
                                     int lddp, void* stream) {
  DV_REQUIRE(pred && x_start && noise && t && sqrt_ac && sqrt_1m_ac && dloss && dpred &&
                 num_timesteps > 0, "bad arguments");
  DV_REQUIRE(objective_ok(objective), "objective is DV_OBJ_EPS, DV_OBJ_X0 or DV_OBJ_V");
  if (objective == DV_OBJ_EPS)
    return dv_mse_loss_bwd(dtype, pred, ld, noise, B, C, T, H, W, sample_w, dloss, dpred, lddp, stream);
  DV_REQUIRE(dtype == DV_F32 || dtype == DV_BF16, "unknown dtype");
  const long long npix = (long long)B * T * H * W;
  const float scale = 1.f / (float)((double)B * C * T * H * W);
  hipStream_t st = (hipStream_t)stream;
#define DV_DLB(TT, OBJ) diff_loss_bwd_kernel<TT, OBJ><<<grid_for(npix), 256, 0, st>>>((const TT*)pred, ld, \
    x_start, noise, t, sqrt_ac, sqrt_1m_ac, B, C, T, H * W, normalize, num_timesteps, sample_w, dloss, scale, \
    (TT*)dpred, lddp)
  if (objective == DV_OBJ_X0) {
    if (dtype == DV_F32) DV_DLB(float, DV_OBJ_X0); else DV_DLB(bf16, DV_OBJ_X0);
  } else {
    if (dtype == DV_F32) DV_DLB(float, DV_OBJ_V); else DV_DLB(bf16, DV_OBJ_V);
  }
#undef DV_DLB
  return check_launch("diffusion_loss_bwd");
}

extern "C" int dv_sinusoidal(const long long* t, const float* freqs, float* out, int B, int dim,
                             void* stream) {
  DV_REQUIRE(t && freqs && out && dim >= 4 && dim % 2 == 0, "bad arguments");
  sinusoidal_kernel<<<grid_for((long long)B * dim), 256, 0, (hipStream_t)stream>>>(t, freqs, out, B, dim);
  return check_launch("sinusoidal");
}

extern "C" int dv_linear_small_fwd(const float* x, int ldx, const float* W, const float* bias,
                                   float* y, int ldy, float* z, int B, int K, int N, int act_in,
                                   int act_out, void* stream) {
  DV_REQUIRE(x && W && y && (act_out != 2 || z), "bad arguments");
  linear_small_kernel<<<(N + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, ldx, W, bias, y, ldy, z, B,
                                                                     K, N, act_in, act_out);
  return check_launch("linear_small_fwd");
}

extern "C" int dv_linear_small_bwd(const float* dy, int lddy, const float* x, int ldx,
                                   const float* W, const float* z, float* dx, int lddx, float* dW,
                                   float* db, int B, int K, int N, int act_in, int act_out,
                                   int accumulate_dx, int accumulate_w, void* stream) {
  DV_REQUIRE(dy && x && W && (act_out != 2 || z), "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DV_REQUIRE(B <= 16, "linear_small supports B <= 16 rows");
  if (dW) linear_small_dw_kernel<<<grid_for((long long)N * K), 256, 0, st>>>(dy, lddy, x, ldx, z, dW, db, B, K, N, act_in, act_out, accumulate_w);
  if (dx) {
    if (!accumulate_dx) zero_f32(dx, (long long)(B - 1) * lddx + K, st);
    dim3 grid((K + 255) / 256, (N + 31) / 32);
    linear_small_dx_kernel<<<grid, 256, 0, st>>>(dy, lddy, x, ldx, W, z, dx, lddx, B, K, N, act_in, act_out);
  }
  return check_launch("linear_small_bwd");
}

extern "C" int dv_adamw(float* p, const float* g, float* m, float* v, long long n, long long n_wd,
                        float lr, float beta1, float beta2, float eps, float wd, float bc1,
                        float bc2_sqrt, const float* clip_coef, void* stream) {
  DV_REQUIRE(p && g && m && v, "null pointer");
  const bool al16 = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                      reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (al16)
    adamw_vec_kernel<<<grid_for((n + 7) / 8, 256, 8192), 256, 0, (hipStream_t)stream>>>(
        p, g, m, v, n, n_wd, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, clip_coef);
  else
    adamw_kernel<<<grid_for(n, 256, 8192), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, n_wd, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, clip_coef);
  return check_launch("adamw");
}

extern "C" int dv_grad_clip_coef(const float* g, long long n, float max_norm, float prescale,
                                 float* ws, void* stream) {
  // ws[1] = update coefficient, ws[2] = gradient norm, ws[4 ..] = per-block
  // partial sums (DV_CLIP_WS_FLOATS in all)
  DV_REQUIRE(g && ws, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = grid_for(n, 256, DV_CLIP_WS_FLOATS - 4);
  sumsq_kernel<<<nb, 256, 0, st>>>(g, n, ws + 4);
  clip_coef_kernel<<<1, 256, 0, st>>>(ws + 4, (int)nb, max_norm, prescale, ws + 1);
  return check_launch("grad_clip_coef");
}

// launches one instantiation of an update kernel: K(T, OBJ, DYN) is the launch.
// eps with the static clamp is the kernel of dv_p_sample / dv_ddim_step
#define DV_UPDATE_DISPATCH(K)                                   \
  do {                                                          \
    if (dtype != DV_F32 && dtype != DV_BF16) DV_REQUIRE(false, "unknown dtype"); \
    const bool f32 = dtype == DV_F32;                           \
    if (objective == DV_OBJ_EPS && !dyn_s) {                    \
      if (f32) K(float, DV_OBJ_EPS, false); else K(bf16, DV_OBJ_EPS, false); \
    } else if (objective == DV_OBJ_EPS) {                       \
      if (f32) K(float, DV_OBJ_EPS, true); else K(bf16, DV_OBJ_EPS, true);   \
    } else if (objective == DV_OBJ_X0) {                        \
      if (f32) K(float, DV_OBJ_X0, true); else K(bf16, DV_OBJ_X0, true);     \
    } else {                                                    \
      if (f32) K(float, DV_OBJ_V, true); else K(bf16, DV_OBJ_V, true);       \
    }                                                           \
  } while (0)

extern "C" int dv_p_sample_obj(int dtype, const float* x, const void* pred, int ld,
                               const float* noise, const long long* t, const float* k_x,
                               const float* k_pred, const float* coef1, const float* coef2,
                               const float* logvar, const float* dyn_s, float* out, float* x0_out,
                               int B, int C, int T, int H, int W, int clip, int objective,
                               int num_timesteps, void* stream) {
  DV_REQUIRE(x && pred && noise && t && out && num_timesteps > 0, "bad arguments");
  DV_REQUIRE(objective_ok(objective), "objective is DV_OBJ_EPS, DV_OBJ_X0 or DV_OBJ_V");
  DV_REQUIRE(objective == DV_OBJ_X0 || (k_x && k_pred), "the eps and v objectives need both x0 tables");
  DV_REQUIRE(!dyn_s || clip, "a dynamic threshold applies only with clip != 0");
  const long long n = (long long)B * C * T * H * W;
  hipStream_t st = (hipStream_t)stream;
#define DV_PS(TT, OBJ, DYN) p_sample_kernel<TT, OBJ, DYN><<<grid_for(n), 256, 0, st>>>(                   \
    x, (const TT*)pred, ld, noise, t, k_x, k_pred, coef1, coef2, logvar, dyn_s, out, x0_out, B, C, T, H * W, \
    clip, num_timesteps)
  DV_UPDATE_DISPATCH(DV_PS);
#undef DV_PS
  return check_launch("p_sample");
}

extern "C" int dv_p_sample(int dtype, const float* x, const void* eps, int ld, const float* noise,
                           const long long* t, const float* sqrt_recip_ac,
                           const float* sqrt_recipm1_ac, const float* coef1, const float* coef2,
                           const float* logvar, float* out, float* x0_out, int B, int C, int T,
                           int H, int W, int clip, int num_timesteps, void* stream) {
  DV_REQUIRE(x && eps && noise && t && out && num_timesteps > 0, "bad arguments");
  const long long n = (long long)B * C * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (p_sample_kernel<float, DV_OBJ_EPS, false><<<grid_for(n), 256, 0, st>>>(x, (const float*)eps, ld, noise, t, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, logvar, nullptr, out, x0_out, B, C, T, H * W, clip, num_timesteps)),
           (p_sample_kernel<bf16, DV_OBJ_EPS, false><<<grid_for(n), 256, 0, st>>>(x, (const bf16*)eps, ld, noise, t, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, logvar, nullptr, out, x0_out, B, C, T, H * W, clip, num_timesteps)));
  return check_launch("p_sample");
}

extern "C" int dv_ddim_step_obj(int dtype, const float* x, const void* pred, int ld,
                                const float* noise, const long long* t, const long long* t_next,
                                const float* alphas_cumprod, float eta, const float* dyn_s,
                                float* out, float* x0_out, int B, int C, int T, int H, int W,
                                int clip, int objective, int num_timesteps, void* stream) {
  DV_REQUIRE(x && pred && t && t_next && alphas_cumprod && out && num_timesteps > 0, "bad arguments");
  DV_REQUIRE(noise || eta == 0.f, "noise may be NULL only when eta == 0");
  DV_REQUIRE(ld == 0 ? dtype == DV_F32 : ld >= C, "pred is NCTHW f32 (ld == 0) or channels-last with ld >= C");
  DV_REQUIRE(objective_ok(objective), "objective is DV_OBJ_EPS, DV_OBJ_X0 or DV_OBJ_V");
  DV_REQUIRE(!dyn_s || clip, "a dynamic threshold applies only with clip != 0");
  const long long n = (long long)B * C * T * H * W;
  hipStream_t st = (hipStream_t)stream;
#define DV_DD(TT, OBJ, DYN) ddim_step_kernel<TT, OBJ, DYN><<<grid_for(n), 256, 0, st>>>(              \
    x, (const TT*)pred, ld, noise, t, t_next, alphas_cumprod, eta, dyn_s, out, x0_out, B, C, T, H * W, \
    clip, num_timesteps)
  DV_UPDATE_DISPATCH(DV_DD);
#undef DV_DD
  return check_launch("ddim_step");
}

extern "C" int dv_ddim_step(int dtype, const float* x, const void* eps, int ld, const float* noise,
                            const long long* t, const long long* t_next,
                            const float* alphas_cumprod, float eta, float* out, float* x0_out,
                            int B, int C, int T, int H, int W, int clip, int num_timesteps,
                            void* stream) {
  DV_REQUIRE(x && eps && t && t_next && alphas_cumprod && out && num_timesteps > 0, "bad arguments");
  DV_REQUIRE(noise || eta == 0.f, "noise may be NULL only when eta == 0");
  DV_REQUIRE(ld == 0 ? dtype == DV_F32 : ld >= C, "eps is NCTHW f32 (ld == 0) or channels-last with ld >= C");
  const long long n = (long long)B * C * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH(dtype,
           (ddim_step_kernel<float, DV_OBJ_EPS, false><<<grid_for(n), 256, 0, st>>>(x, (const float*)eps, ld, noise, t, t_next, alphas_cumprod, eta, nullptr, out, x0_out, B, C, T, H * W, clip, num_timesteps)),
           (ddim_step_kernel<bf16, DV_OBJ_EPS, false><<<grid_for(n), 256, 0, st>>>(x, (const bf16*)eps, ld, noise, t, t_next, alphas_cumprod, eta, nullptr, out, x0_out, B, C, T, H * W, clip, num_timesteps)));
  return check_launch("ddim_step");
}

// ---- inpainting (ABI 9) ----

extern "C" int dv_inpaint_blend(float* x, const float* known, const unsigned char* mask,
                                const float* noise, const long long* t, const long long* t_from,
                                const float* sqrt_ac, const float* sqrt_1m_ac, int B, int C, int T,
                                int H, int W, int normalize, int final, int num_timesteps,
                                void* stream) {
  DV_REQUIRE(x && known && mask && B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "bad arguments");
  DV_REQUIRE(final || (noise && t && sqrt_ac && sqrt_1m_ac && num_timesteps > 0),
             "noise, t and both tables may be NULL only with final != 0");
  DV_REQUIRE(!(final && t_from), "the final blend takes no t_from");
  DV_REQUIRE((long long)H * W <= 0x7fffffffLL, "H * W must fit an int");
  const int HW = H * W;
  const long long n = (long long)B * C * T * HW;
  const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(known) |
                       reinterpret_cast<uintptr_t>(noise);
  const bool vec = HW % 4 == 0 && (al & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
#define DV_IB(VEC, FINAL) inpaint_blend_kernel<VEC, FINAL><<<grid_for(n / (VEC ? 4 : 1), 256, 2048), 256, 0, st>>>( \
    x, known, mask, noise, t, t_from, sqrt_ac, sqrt_1m_ac, B, C, T, HW, normalize, num_timesteps)
  if (vec) {
    if (final) DV_IB(true, true); else DV_IB(true, false);
  } else {
    if (final) DV_IB(false, true); else DV_IB(false, false);
  }
#undef DV_IB
  return check_launch("inpaint_blend");
}

// ---- self-conditioning (ABI 8) ----

static bool dtype_ok(int d) { return d == DV_F32 || d == DV_BF16; }

extern "C" int dv_q_sample_sc(int dtype, const float* x0, const float* noise, const long long* t,
                              const float* sqrt_ac, const float* sqrt_1m_ac, const void* self_cond,
                              int ldsc, int sc_dtype, void* y, int B, int C, int Csc, int T, int H,
                              int W, int cpad, int normalize, int num_timesteps, void* stream) {
  DV_REQUIRE(x0 && noise && t && sqrt_ac && sqrt_1m_ac && y && num_timesteps > 0 && B > 0 && C > 0 &&
                 T > 0 && H > 0 && W > 0 && Csc >= 0,
             "bad arguments");
  DV_REQUIRE(dtype_ok(dtype), "unknown dtype");
  DV_REQUIRE(cpad % 8 == 0 && (long long)C + Csc <= cpad, "C + Csc <= cpad and cpad % 8 == 0");
  DV_REQUIRE(!self_cond || (dtype_ok(sc_dtype) && ldsc >= Csc), "self_cond is channels-last f32 / bf16 with ldsc >= Csc");
  DV_REQUIRE((uintptr_t)y % 16 == 0, "y must be 16-byte aligned");
  const long long npix = (long long)B * T * H * W;
  hipStream_t st = (hipStream_t)stream;
  const int scb = sc_dtype == DV_BF16;
  if (dtype == DV_F32)
    q_sample_sc_kernel<float><<<grid_for(npix), 256, 0, st>>>(x0, noise, t, sqrt_ac, sqrt_1m_ac, self_cond, ldsc, scb, (float*)y, B, C, Csc, T, H * W, cpad, normalize, num_timesteps);
  else
    q_sample_sc_kernel<bf16><<<grid_for(npix), 256, 0, st>>>(x0, noise, t, sqrt_ac, sqrt_1m_ac, self_cond, ldsc, scb, (bf16*)y, B, C, Csc, T, H * W, cpad, normalize, num_timesteps);
  return check_launch("q_sample_sc");
}

extern "C" int dv_dyn_thres(int dtype, const float* x, const void* pred, int ld, const long long* t,
                            const float* k_x, const float* k_pred, int B, int C, int T, int H, int W,
                            int objective, int num_timesteps, long long k0, float frac, float* s,
                            void* stream) {
  DV_REQUIRE(x && pred && t && s && num_timesteps > 0 && B > 0 && C > 0 && T > 0 && H > 0 && W > 0,
             "bad arguments");
  DV_REQUIRE(ld == 0 ? dtype == DV_F32 : ld >= C, "pred is NCTHW f32 (ld == 0) or channels-last with ld >= C");
  DV_REQUIRE(dtype == DV_F32 || dtype == DV_BF16, "unknown dtype");
  DV_REQUIRE(objective_ok(objective), "objective is DV_OBJ_EPS, DV_OBJ_X0 or DV_OBJ_V");
  DV_REQUIRE(objective == DV_OBJ_X0 || k_x, "the eps and v objectives need k_x (with k_pred == NULL: alphas_cumprod)");
  const long long N = (long long)C * T * H * W;
  DV_REQUIRE(N < (1ll << 31), "more than 2^31 - 1 elements per sample");
  DV_REQUIRE(k0 >= 0 && k0 < N && frac >= 0.f && frac < 1.f && (frac == 0.f || k0 + 1 < N),
             "the quantile position k0 + frac lies outside [0, N - 1]");
  hipStream_t st = (hipStream_t)stream;
#define DV_DT(TT, OBJ) dyn_thres_kernel<TT, OBJ><<<B, DT_THREADS, 0, st>>>(                     \
    x, (const TT*)pred, ld, t, k_x, k_pred, C, T * H, W, num_timesteps, k0, frac, s)
#define DV_DT_T(OBJ)                      \
  if (dtype == DV_F32) DV_DT(float, OBJ); \
  else DV_DT(bf16, OBJ)
  if (objective == DV_OBJ_EPS) { DV_DT_T(DV_OBJ_EPS); }
  else if (objective == DV_OBJ_X0) { DV_DT_T(DV_OBJ_X0); }
  else { DV_DT_T(DV_OBJ_V); }
#undef DV_DT_T
#undef DV_DT
  return check_launch("dyn_thres");
}

extern "C" int dv_resize_nearest(const float* x, float* y, long long planes, int hin, int win,
                                 int hout, int wout, int do_clamp, float lo, float hi,
                                 void* stream) {
  DV_REQUIRE(x && y && hin > 0 && win > 0 && hout > 0 && wout > 0, "bad arguments");
  resize_nearest_kernel<<<grid_for(planes * hout * wout), 256, 0, (hipStream_t)stream>>>(
      x, y, planes, hin, win, hout, wout, do_clamp, lo, hi);
  return check_launch("resize_nearest");
}

extern "C" int dv_gaussian_blur(const float* x, float* y, long long planes, int H, int W, int ks,
                                const float* w1, void* stream) {
  DV_REQUIRE(x && y && w1 && (ks & 1) && ks / 2 < H && ks / 2 < W, "bad arguments");
  blur_kernel<<<grid_for(planes * H * W), 256, 0, (hipStream_t)stream>>>(x, y, planes, H, W, ks, w1);
  return check_launch("gaussian_blur");
}

static int linear_group(bool bwd, const float* x, int B, int K, int act_in, const DvLinEntry* entries,
                        int n_entries, float* dx, int accumulate_dx, float* ws, hipStream_t st) {
  bool any = false;
  for (int s0 = 0; s0 < n_entries; s0 += LG_MAX) {
    LinGroupArgs a;
    a.x = x; a.dx = dx; a.ws = ws; a.B = B; a.K = K; a.act_in = act_in; a.acc_dx = accumulate_dx;
    a.n = n_entries - s0 < LG_MAX ? n_entries - s0 : LG_MAX;
    a.finalize = s0 + LG_MAX >= n_entries;
    int blk = 0;
    for (int i = 0; i < a.n; ++i) {
      a.e[i] = entries[s0 + i];
      a.blk0[i] = blk;
      blk += (entries[s0 + i].n + LG_ROWS - 1) / LG_ROWS;
    }
    a.blk0[a.n] = blk;
    if (blk == 0) continue;
    any = true;
    if (bwd) linear_group_bwd_kernel<<<blk, 256, 0, st>>>(a);
    else linear_group_fwd_kernel<<<blk, 256, 0, st>>>(a);
  }
  if (bwd && dx && !any) {  // no rows at all: dx gets nothing (still honour accumulate)
    if (!accumulate_dx) zero_f32(dx, (long long)B * K, st);
  }
  return check_launch(bwd ? "linear_group_bwd" : "linear_group_fwd");
}

static const char* lg_validate(const float* x, int B, int K, const DvLinEntry* entries,
                               int n_entries) {
  if (!x || !entries || n_entries < 0) return "null pointer";
  if (B < 1 || B > LG_MAXB || K < 4 || K > LG_MAXK || K % 4 != 0)
    return "need 1 <= B <= 8, K % 4 == 0, K <= 512";
  for (int i = 0; i < n_entries; ++i)
    if (!entries[i].w || !entries[i].y || entries[i].n < 0) return "bad entry";
  return nullptr;
}

extern "C" int dv_linear_group_fwd(const float* x, int B, int K, int act_in, const DvLinEntry* entries,
                                   int n_entries, void* stream) {
  const char* bad = lg_validate(x, B, K, entries, n_entries);
  DV_REQUIRE(!bad, bad ? bad : "");
  return linear_group(false, x, B, K, act_in, entries, n_entries, nullptr, 0, nullptr,
                      (hipStream_t)stream);
}

extern "C" int dv_linear_group_bwd(const float* x, int B, int K, int act_in, const DvLinEntry* entries,
                                   int n_entries, float* dx, int accumulate_dx, float* ws,
                                   void* stream) {
  const char* bad = lg_validate(x, B, K, entries, n_entries);
  DV_REQUIRE(!bad, bad ? bad : "");
  DV_REQUIRE(!dx || ws, "backward dx needs ws");
  return linear_group(true, x, B, K, act_in, entries, n_entries, dx, accumulate_dx, ws,
                      (hipStream_t)stream);
}
