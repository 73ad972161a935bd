// Channels-last ([M, C] view of NDHWC / NHWC activations) BatchNorm, global average pool and the NCDHW -> NDHWC
// video copy, shared by the R3D-18 (cmhar/r3d.py) and 2-D CNN (cmhar/cnn2d.py) backbones.  BatchNorm (training batch
// statistics, eps / momentum as nn.BatchNorm3d) is a two-level deterministic column reduction over the [M, C] view —
// or the combination of the per-tile statistics a conv epilogue of conv3d.hip already wrote — plus an apply pass
// that fuses the residual add and ReLU of torchvision's BasicBlock; its backward fuses the ReLU mask and emits the
// residual-branch gradient.
#include "channels_last.h"

namespace {

// ---- BatchNorm over the [M, C] channels-last view ----------------------------------------------------------------
// Column partial sums over a chunk of rows: each thread reads 8 consecutive channels of a row (one 16-B bf16
// vector), TPR = C/8 threads cover a row and the block's RPI = 256/TPR row slots are combined in a fixed order.
// mode 0: Σx; mode 1: Σ(x−mean)²; mode 2: Σg, Σg·x̂ with g = dy·act'(y) (relu 1: [y > 0]; relu 2 = ReLU6:
// [0 < y < 6]).  part: [2][nchunk][C].  C/8 need not divide 256: the 256 % TPR spare threads only add zeros.
// relu | BN_ZMASK: the unit had no residual input, so y = act(x̂·w + b) is recomputed from x in bn_cl_apply's exact
// arithmetic and rounding (bit-identical mask) instead of read: one M×C tensor less per pass.
constexpr int BN_ZMASK = 4;
// act'(y) ≠ 0 from the stored y: ReLU [y > 0] (+inf included, as torch's threshold_backward on the result), ReLU6
// [0 < y < 6]; NaN → 0.
__device__ __forceinline__ bool bn_y_on(float y, int relu) { return y > 0.f && ((relu & 3) != 2 || y < 6.f); }
// The same mask from the pre-activation v = fmaf((x − mean)·rstd, w, b) (bn_cl_apply's arithmetic), without the
// round trip y = T(clamp(v)): for bf16 storage T(v) of 0 < v ≤ 2^-134 is +0 (round to nearest even: 2^-134 is the
// tie between +0 and the smallest denormal 2^-133) and ReLU6's T(v) reaches 6 from v = 6 − 2^-6 on (the tie rounds
// to the even 6.0); fp32 storage keeps v.  NaN: the forward's clamp gives 0 → off, as here.
template <typename T>
__device__ __forceinline__ bool bn_act_on(float v, int relu) {
  constexpr bool B16 = sizeof(T) == 2;
  return v > (B16 ? 0x1p-134f : 0.f) && ((relu & 3) != 2 || v < (B16 ? 5.984375f : 6.f));
}
template <typename T, int MODE, bool ZM = false>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 4 : 3) void bn_cl_partial(int M, int C, int rows_per_chunk, const T* __restrict__ x,
                                                     const T* __restrict__ y, const T* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ w, const float* __restrict__ b,
                                                     int relu, float* __restrict__ part) {
  static_assert(MODE >= 0 && MODE <= 2 && (!ZM || MODE == 2), "modes 0 / 1 / 2; the z-mask in mode 2 only");
  __shared__ float s0[256][9], s1[256][9];
  const int tid = threadIdx.x;
  const int TPR = C / 8, RPI = 256 / TPR;
  const int slot = tid / TPR, c0 = (tid % TPR) * 8;
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(r0 + rows_per_chunk, M);
  const int rs0 = slot < RPI ? r0 + slot : r1;
  // ZM: a separate instantiation (the mask's w / b and the y loads never share registers); bf16: ≤ 128 VGPRs (launch
  // bounds), 4 waves per SIMD, the 1024 chunks of bn_chunks in one round; MODE compile-time: one loop body
  const bool ry = !ZM && MODE == 2 && relu;
  float mu[8], rs[8], a0[8], a1[8], ww[8], bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = MODE ? mean[c0 + j] : 0.f;
    rs[j] = MODE == 2 ? rstd[c0 + j] : 0.f;
    ww[j] = ZM ? w[c0 + j] : 0.f;
    bb[j] = ZM ? b[c0 + j] : 0.f;
    a0[j] = a1[j] = 0.f;
  }
  auto accum = [&](const float* v, const float* gv, const float* yv) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (MODE == 0) {
        a0[j] += v[j];
      } else if (MODE == 1) {
        const float d = v[j] - mu[j];
        a0[j] = fmaf(d, d, a0[j]);
      } else {
        const float xh = (v[j] - mu[j]) * rs[j];
        const bool off = ZM ? !bn_act_on<T>(fmaf(xh, ww[j], bb[j]), relu) : relu && !bn_y_on(yv[j], relu);
        const float gj = off ? 0.f : gv[j];
        a0[j] += gj;
        a1[j] = fmaf(gj, xh, a1[j]);
      }
    }
  };
  // four row slots' loads in flight per thread (with 2–3 waves per SIMD one 16-B load per tensor left the kernel at
  // ~1.5 TB/s), accumulated in the same sequential row order as the one-row tail loop
  constexpr int UR = 4;
  int r = rs0;
  for (; r + (UR - 1) * RPI < r1; r += UR * RPI) {
    float v[UR][8], gv[UR][8], yv[UR][8];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long off = (long)(r + u * RPI) * C + c0;
      Vec8<T>::load(x + off, v[u]);
      if (MODE == 2) {
        Vec8<T>::load(dy + off, gv[u]);
        if (ry) Vec8<T>::load(y + off, yv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) accum(v[u], gv[u], yv[u]);
  }
  for (; r < r1; r += RPI) {
    const long off = (long)r * C + c0;
    float v[8], gv[8], yv[8];
    Vec8<T>::load(x + off, v);
    if (MODE == 2) {
      Vec8<T>::load(dy + off, gv);
      if (ry) Vec8<T>::load(y + off, yv);
    }
    accum(v, gv, yv);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { s0[tid][j] = a0[j]; s1[tid][j] = a1[j]; }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float b0 = 0.f, b1 = 0.f;
    for (int sl = 0; sl < RPI; ++sl) { b0 += s0[sl * TPR + c / 8][c % 8]; b1 += s1[sl * TPR + c / 8][c % 8]; }
    part[(long)blockIdx.x * C + c] = b0;
    if (MODE == 2) part[((long)gridDim.x + blockIdx.x) * C + c] = b1;
  }
}

// Combine the chunk partials (BN_FC columns per block, 256 / BN_FC chunk slots, fixed order) and finish the statistic.
// mode 0: mean;  mode 1: rstd (+ running stats, num_batches_tracked);  mode 2: db = Σg, dw = Σg·x̂.
// Each slot keeps BN_FU independent partial sums (BN_FU chunk loads in flight instead of one dependent chain; the
// kernel is load-latency bound: ≤ 512 KiB of partials), combined in a fixed order.
constexpr int BN_FC = 4, BN_FS = 256 / BN_FC, BN_FU = 4;
static_assert(BN_FU == 4, "the fixed-order combine below adds four partial sums");
__global__ __launch_bounds__(256) void bn_cl_final(int mode, long M, int C, int nchunk, const float* __restrict__ part,
                                                   float* __restrict__ mean, float* __restrict__ rstd,
                                                   float* __restrict__ rmean, float* __restrict__ rvar,
                                                   long long* __restrict__ nbt, float momentum, float eps,
                                                   float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float s0[256], s1[256];
  const int tid = threadIdx.x, cl = tid % BN_FC, slot = tid / BN_FC;
  const int c = blockIdx.x * BN_FC + cl;
  float a0[BN_FU] = {}, a1[BN_FU] = {};
  if (c < C) {
    int k = slot;
    for (; k + (BN_FU - 1) * BN_FS < nchunk; k += BN_FU * BN_FS) {
#pragma unroll
      for (int u = 0; u < BN_FU; ++u) {
        a0[u] += part[(long)(k + u * BN_FS) * C + c];
        if (mode == 2) a1[u] += part[((long)nchunk + k + u * BN_FS) * C + c];
      }
    }
    for (; k < nchunk; k += BN_FS) {
      a0[0] += part[(long)k * C + c];
      if (mode == 2) a1[0] += part[((long)nchunk + k) * C + c];
    }
  }
  s0[tid] = (a0[0] + a0[1]) + (a0[2] + a0[3]);
  s1[tid] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
  __syncthreads();
  if (slot || c >= C) return;
  float b0 = 0.f, b1 = 0.f;
  for (int s = 0; s < BN_FS; ++s) {
    b0 += s0[s * BN_FC + cl];
    b1 += s1[s * BN_FC + cl];
  }
  if (mode == 0) {
    mean[c] = b0 / (float)M;
  } else if (mode == 1) {
    const float var = b0 / (float)M;
    rstd[c] = rsqrtf(var + eps);
    if (rmean) {
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean[c];
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * var * ((float)M / (float)(M > 1 ? M - 1 : 1));
    }
    if (nbt && c == 0) *nbt += 1;
  } else {
    db[c] = b0;
    dw[c] = b1;
  }
}

// Combine per-tile (n_t, mean_t, M2_t) over the ntile row tiles written by a conv epilogue (their row counts n_t in
// `cnt`: 128-row tiles for the generic / 256-row kernels, whole-output-row tiles for the nine-tap forward) with Chan's
// formula, in a fixed order: mean = Σ n_t·mean_t / M,  M2 = Σ M2_t + n_t·(mean_t − mean)².  Then rstd and the
// running statistics as bn_cl_final.  The statistics buffer's layout is tile_stats_layout's (channels_last.h).
// Level 1: one thread per (group of BN_TG tiles, channel) merges its tiles sequentially (Chan's update) into the
// group's (mean, M2); channel 0's thread also writes the group's row count.  The group's loads are issued up front
// (clamped tile index, count 0 past the end) so the sequential merge is not a chain of dependent load latencies.
__global__ __launch_bounds__(256) void bn_tile_group(int C, int ntile, const float* __restrict__ ts,
                                                     const float* __restrict__ cnt, float* __restrict__ out,
                                                     float* __restrict__ gcnt) {
  const int ngroup = (ntile + BN_TG - 1) / BN_TG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)ngroup * C) return;
  const int g = (int)(i / C), c = (int)(i % C);
  float nv[BN_TG], mv[BN_TG], qv[BN_TG];
#pragma unroll
  for (int j = 0; j < BN_TG; ++j) {
    const int t = min(g * BN_TG + j, ntile - 1);
    nv[j] = g * BN_TG + j < ntile ? cnt[t] : 0.f;
    mv[j] = ts[(long)t * C + c];
    qv[j] = ts[((long)ntile + t) * C + c];
  }
  float n = 0.f, mu = 0.f, m2 = 0.f;
#pragma unroll
  for (int j = 0; j < BN_TG; ++j) {
    const float nt = nv[j];
    if (nt <= 0.f) continue;
    const float d = mv[j] - mu, n2 = n + nt;
    mu = fmaf(d, nt / n2, mu);
    m2 += qv[j] + d * d * (n * nt / n2);
    n = n2;
  }
  out[(long)g * C + c] = mu;
  out[((long)ngroup + g) * C + c] = m2;
  if (c == 0) gcnt[g] = n;
}

// Level 2 over the groups (their row counts in gcnt): BN_GC channels per block, BN_GS group slots, each slot with
// BN_FU independent partial sums (fixed-order combine).
constexpr int BN_GC = 4, BN_GS = 256 / BN_GC;
__global__ __launch_bounds__(256) void bn_tile_final(long M, int C, int ngroup, const float* __restrict__ ts,
                                                     const float* __restrict__ gcnt, float* __restrict__ mean,
                                                     float* __restrict__ rstd, float* __restrict__ rmean,
                                                     float* __restrict__ rvar, long long* __restrict__ nbt,
                                                     float momentum, float eps) {
  __shared__ float sh[256];
  __shared__ float smu[BN_GC];
  const int tid = threadIdx.x, cl = tid % BN_GC, slot = tid / BN_GC;
  const int c = blockIdx.x * BN_GC + cl;
  // pass 1: Σ n_g·mean_g;  pass 2: Σ M2_g + n_g·(mean_g − mean)²
  auto sweep = [&](bool second, float mu) {
    float a[BN_FU] = {};
    if (c < C) {
      int t = slot;
      for (; t + (BN_FU - 1) * BN_GS < ngroup; t += BN_FU * BN_GS) {
#pragma unroll
        for (int u = 0; u < BN_FU; ++u) {
          const int tt = t + u * BN_GS;
          const float m = ts[(long)tt * C + c], n = gcnt[tt];
          if (second) {
            const float d = m - mu;
            a[u] += ts[((long)ngroup + tt) * C + c] + n * d * d;
          } else {
            a[u] = fmaf(n, m, a[u]);
          }
        }
      }
      for (; t < ngroup; t += BN_GS) {
        const float m = ts[(long)t * C + c], n = gcnt[t];
        if (second) {
          const float d = m - mu;
          a[0] += ts[((long)ngroup + t) * C + c] + n * d * d;
        } else {
          a[0] = fmaf(n, m, a[0]);
        }
      }
    }
    return (a[0] + a[1]) + (a[2] + a[3]);
  };
  sh[tid] = sweep(false, 0.f);
  __syncthreads();
  if (slot == 0) {
    float b = 0.f;
    for (int k = 0; k < BN_GS; ++k) b += sh[k * BN_GC + cl];
    smu[cl] = b / (float)M;
  }
  __syncthreads();
  const float mu = smu[cl];
  const float q = sweep(true, mu);
  __syncthreads();
  sh[tid] = q;
  __syncthreads();
  if (slot || c >= C) return;
  float m2 = 0.f;
  for (int k = 0; k < BN_GS; ++k) m2 += sh[k * BN_GC + cl];
  const float var = m2 / (float)M;
  mean[c] = mu;
  rstd[c] = rsqrtf(var + eps);
  if (rmean) {
    rmean[c] = (1.f - momentum) * rmean[c] + momentum * mu;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * var * ((float)M / (float)(M > 1 ? M - 1 : 1));
  }
  if (nbt && c == 0) *nbt += 1;
}

__global__ void bn_cl_eval_stats(int C, const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                 float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) { mean[c] = rmean[c]; rstd[c] = rsqrtf(rvar[c] + eps); }
}

// y = act((x − mean)·rstd·w + b + res), act = identity / ReLU (relu 1) / ReLU6 (relu 2), 8 channels per thread.
// HOIST (C/8 divides 256, so a thread's channels never change along the grid-stride loop): the per-channel
// constants are loaded once per thread instead of once per vector (8 of the 10 loads of an iteration).
template <typename T, bool HOIST>
__global__ __launch_bounds__(256) void bn_cl_apply(unsigned nvec, int C, const T* __restrict__ x,
                                                   const T* __restrict__ res, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, const float* __restrict__ w,
                                                   const float* __restrict__ b, int relu, T* __restrict__ y) {
  const unsigned cv = C / 8;
  float mu[8], rs[8], ww[8], bb[8];
  // per-channel constants as explicit 16-B loads (c0 % 8 == 0; the per-element form lost its vectorisation
  // once the activation became a two-way choice: 34 vs 10 loads per 8 channels, 4x slower)
  auto consts = [&](unsigned i) {
    const int c0 = (int)(i % cv) * 8;
    Vec8<float>::load(mean + c0, mu);
    Vec8<float>::load(rstd + c0, rs);
    Vec8<float>::load(w + c0, ww);
    Vec8<float>::load(b + c0, bb);
  };
  const unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (HOIST) consts(i0);
  const float lo = relu ? 0.f : -INFINITY, hi = relu == 2 ? 6.f : INFINITY;
  for (unsigned i = i0; i < nvec; i += gridDim.x * blockDim.x) {
    const long off = (long)i * 8;
    float v[8], rv[8];
    Vec8<T>::load(x + off, v);
    if (res) Vec8<T>::load(res + off, rv);
    if (!HOIST) consts(i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = fmaf((v[j] - mu[j]) * rs[j], ww[j], bb[j]);
      if (res) v[j] += rv[j];
      v[j] = fminf(fmaxf(v[j], lo), hi);
    }
    Vec8<T>::store(y + off, v);
  }
}

// g = dy·act'(y);  dres = g (optional);  dx = w·rstd·(g − Σg/M − x̂·Σgx̂/M) (training) or w·rstd·g (eval).
// relu | BN_ZMASK: act'(y) recomputed from x (no residual; see bn_cl_partial), y not read.  HOIST: as bn_cl_apply.
template <typename T, bool HOIST>
__global__ __launch_bounds__(256) void bn_cl_bwd_apply(unsigned nvec, int M, int C, const T* __restrict__ x,
                                                       const T* __restrict__ y, const T* __restrict__ dy,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       const float* __restrict__ dw, const float* __restrict__ db,
                                                       int training, int relu, T* __restrict__ dx,
                                                       T* __restrict__ dres) {
  const float inv = 1.f / (float)M;
  const unsigned cv = C / 8;
  const bool zm = relu & BN_ZMASK, ry = relu && !zm, needx = training || zm;
  float rs[8], ww[8], mu[8], sw[8], sb[8], bb[8];
  // per-channel constants as explicit 16-B loads (c0 % 8 == 0): per element they compiled to 40 scalar loads
  auto consts = [&](unsigned i) {
    const int c0 = (int)(i % cv) * 8;
    Vec8<float>::load(rstd + c0, rs);
    Vec8<float>::load(w + c0, ww);
    if (needx) Vec8<float>::load(mean + c0, mu);
    if (training) {
      Vec8<float>::load(dw + c0, sw);
      Vec8<float>::load(db + c0, sb);
    }
    if (zm) Vec8<float>::load(b + c0, bb);
  };
  const unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (HOIST) consts(i0);
  for (unsigned i = i0; i < nvec; i += gridDim.x * blockDim.x) {
    const long off = (long)i * 8;
    float gv[8], yv[8], xv[8], out[8];
    Vec8<T>::load(dy + off, gv);
    if (ry) Vec8<T>::load(y + off, yv);
    if (needx) Vec8<T>::load(x + off, xv);
    if (!HOIST) consts(i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (zm ? !bn_act_on<T>(fmaf((xv[j] - mu[j]) * rs[j], ww[j], bb[j]), relu) : ry && !bn_y_on(yv[j], relu))
        gv[j] = 0.f;
      if (training) {
        const float xh = (xv[j] - mu[j]) * rs[j];
        out[j] = ww[j] * rs[j] * (gv[j] - sb[j] * inv - xh * sw[j] * inv);
      } else {
        out[j] = ww[j] * rs[j] * gv[j];
      }
    }
    if (dres) Vec8<T>::store(dres + off, gv);
    Vec8<T>::store(dx + off, out);
  }
}

// Global average pool over the S positions of each clip: [N, S, C] → fp32 [N, C]; backward broadcasts dout/S.
template <typename T>
__global__ __launch_bounds__(256) void avgpool_cl_fwd(int N, long S, int C, const T* __restrict__ x,
                                                      float* __restrict__ out) {
  __shared__ float sh[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int CB = C < 256 ? C : 256, RPI = 256 / CB, slot = tid / CB, cc = tid % CB;
  for (int c0 = blockIdx.x * CB; c0 < C; c0 += gridDim.x * CB) {
    float a = 0.f;
    if (slot < RPI && c0 + cc < C)      // (C not a multiple of CB / CB not dividing 256: spare threads add 0)
      for (long s = slot; s < S; s += RPI) a += to_f<T>(x[((long)n * S + s) * C + c0 + cc]);
    sh[tid] = a;
    __syncthreads();
    if (slot == 0 && c0 + cc < C) {
      float b = 0.f;
      for (int k = 0; k < RPI; ++k) b += sh[k * CB + cc];
      out[(long)n * C + c0 + cc] = b / (float)S;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_cl_bwd(long total, long S, int C, const float* __restrict__ dout,
                                                      T* __restrict__ dx) {
  const float inv = 1.f / (float)S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long n = i / C / S;
    dx[i] = from_f<T>(dout[n * C + c] * inv);
  }
}

// (B, T, C, H, W) fp32 video → (B, T, H, W, C) compute dtype.
template <typename T>
__global__ __launch_bounds__(256) void video_ndhwc_kernel(long total, int C, long HW, const float* __restrict__ v,
                                                          T* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long p = i / C;          // (b·T + t)·HW + hw
    const long bt = p / HW, hw = p - bt * HW;
    out[i] = from_f<T>(v[(bt * C + c) * HW + hw]);
  }
}

inline bool bn_channels_ok(int C) { return C >= 8 && C % 8 == 0 && C <= 2048; }

// ≤ 1024 chunks of ≥ 16 K elements per tensor: four blocks per CU stream the big R3D-18 layers (M·C = 103 M at
// 16×56², where ≤ 512 chunks of ≥ 512 rows ran 1.5 TB/s), a few blocks the 7² layer-4 maps; few partials to combine
inline int bn_chunks(long M, int C) {
  const long c = (M * C + 16383) / 16384;
  return (int)(c < 1024 ? (c > 0 ? c : 1) : 1024);
}

}  // namespace

// A thread's 8 channels are fixed along the grid-stride loop when C/8 divides 256 (grid_for's blocks are 256 wide)
inline bool bn_hoist(int C) { return 256 % (C / 8) == 0; }

template <typename T>
void bn_apply_launch(long M, int C, const void* x, const void* res, const float* smean, const float* srstd,
                     const float* w, const float* b, int relu, void* y, hipStream_t stream) {
  const unsigned nvec = (unsigned)(M * C / 8);
  if (bn_hoist(C))
    bn_cl_apply<T, true><<<grid_for(nvec), 256, 0, stream>>>(nvec, C, (const T*)x, (const T*)res, smean, srstd, w,
                                                              b, relu, (T*)y);
  else
    bn_cl_apply<T, false><<<grid_for(nvec), 256, 0, stream>>>(nvec, C, (const T*)x, (const T*)res, smean, srstd, w,
                                                               b, relu, (T*)y);
}

// BatchNorm backward: column partials (Σg, Σg·x̂), their combination into db / dw, then dx (and dres).
// y == nullptr with relu != 0: no residual entered the unit, the activation mask is recomputed from x (BN_ZMASK).
template <typename T>
int bn_bwd_launch(long M, int C, const void* x, const void* y, const void* dy, const float* w, const float* b,
                  const float* smean, const float* srstd, void* dx, void* dres, float* dw, float* db, int training,
                  int relu, float* ws, hipStream_t stream) {
  const int nch = bn_chunks(M, C);
  const int rpc = (int)((M + nch - 1) / nch);
  const int act = relu && !y ? relu | BN_ZMASK : relu;
  if (act & BN_ZMASK)
    bn_cl_partial<T, 2, true><<<nch, 256, 0, stream>>>((int)M, C, rpc, (const T*)x, (const T*)y, (const T*)dy, smean,
                                                     srstd, w, b, act, ws);
  else
    bn_cl_partial<T, 2, false><<<nch, 256, 0, stream>>>((int)M, C, rpc, (const T*)x, (const T*)y, (const T*)dy,
                                                      smean, srstd, w, b, act, ws);
  bn_cl_final<<<(C + BN_FC - 1) / BN_FC, 256, 0, stream>>>(2, M, C, nch, ws, nullptr, nullptr, nullptr, nullptr,
                                                           nullptr, 0.f, 0.f, dw, db);
  const unsigned nvec = (unsigned)(M * C / 8);
  if (bn_hoist(C))
    bn_cl_bwd_apply<T, true><<<grid_for(nvec), 256, 0, stream>>>(nvec, (int)M, C, (const T*)x, (const T*)y,
                                                                  (const T*)dy, smean, srstd, w, b, dw, db, training,
                                                                  act, (T*)dx, (T*)dres);
  else
    bn_cl_bwd_apply<T, false><<<grid_for(nvec), 256, 0, stream>>>(nvec, (int)M, C, (const T*)x, (const T*)y,
                                                                   (const T*)dy, smean, srstd, w, b, dw, db, training,
                                                                   act, (T*)dx, (T*)dres);
  return 0;
}

extern "C" long cmhar_bn_cl_ws(long M, int C) { return 2L * bn_chunks(M, C) * C; }

extern "C" int cmhar_bn_cl_fwd(int dtype, long M, int C, const void* x, const void* res, void* y, const float* w,
                               const float* b, float* rmean, float* rvar, float* smean, float* srstd, int training,
                               float momentum, float eps, int relu, long long* num_batches_tracked, float* ws,
                               hipStream_t stream) {
  if (M <= 0 || !bn_channels_ok(C) || !ws) return -1;
  if (M >= (1L << 31) || M * C / 8 >= (1L << 31)) return -2;   // unsigned grid-stride loops never wrap
  const int nch = bn_chunks(M, C);
  const int rpc = (int)((M + nch - 1) / nch);
  const int fgrid = (C + BN_FC - 1) / BN_FC;
  if (training) {
    for (int mode = 0; mode < 2; ++mode) {
#define BNP(T, MODE)                                                                                            \
  bn_cl_partial<T, MODE><<<nch, 256, 0, stream>>>((int)M, C, rpc, (const T*)x, nullptr, nullptr, smean, nullptr,  \
                                                  nullptr, nullptr, 0, ws)
      if (dtype == CMHAR_BF16) {
        if (mode == 0) BNP(bf16, 0);
        else BNP(bf16, 1);
      } else if (dtype == CMHAR_F32) {
        if (mode == 0) BNP(float, 0);
        else BNP(float, 1);
      } else return -1;
#undef BNP
      bn_cl_final<<<fgrid, 256, 0, stream>>>(mode, M, C, nch, ws, smean, srstd, rmean, rvar, num_batches_tracked,
                                             momentum, eps, nullptr, nullptr);
    }
  } else {
    if (!rmean || !rvar) return -2;
    bn_cl_eval_stats<<<(C + 255) / 256, 256, 0, stream>>>(C, rmean, rvar, eps, smean, srstd);
  }
  if (dtype == CMHAR_BF16) bn_apply_launch<bf16>(M, C, x, res, smean, srstd, w, b, relu, y, stream);
  else bn_apply_launch<float>(M, C, x, res, smean, srstd, w, b, relu, y, stream);
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_bn_cl_fwd_tiles(long M, int C, int ntile, float* tile_stats, const void* x, const void* res,
                                     void* y, const float* w, const float* b, float* rmean, float* rvar,
                                     float* smean, float* srstd, float momentum, float eps, int relu,
                                     long long* num_batches_tracked, hipStream_t stream) {
  if (M <= 0 || !bn_channels_ok(C) || !tile_stats || ntile <= 0) return -1;
  if (M >= (1L << 31) || M * C / 8 >= (1L << 31)) return -2;   // unsigned grid-stride loops never wrap
  const TileStats ts = tile_stats_layout(ntile, C);
  float* groups = tile_stats + ts.groups;
  float* gcnt = tile_stats + ts.gcnt;
  bn_tile_group<<<cdiv((long)ts.ngroup * C, 256), 256, 0, stream>>>(C, ntile, tile_stats, tile_stats + ts.cnt, groups,
                                                                    gcnt);
  bn_tile_final<<<(C + BN_GC - 1) / BN_GC, 256, 0, stream>>>(M, C, ts.ngroup, groups, gcnt, smean, srstd, rmean, rvar,
                                                             num_batches_tracked, momentum, eps);
  bn_apply_launch<bf16>(M, C, x, res, smean, srstd, w, b, relu, y, stream);
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_bn_cl_bwd(int dtype, long M, int C, const void* x, const void* y, const void* dy,
                               const float* w, const float* smean, const float* srstd, void* dx, void* dres,
                               float* dw, float* db, int training, int relu, float* ws, hipStream_t stream) {
  if (M <= 0 || !bn_channels_ok(C) || !ws || !dw || !db || (relu && !y)) return -1;
  if (M >= (1L << 31) || M * C / 8 >= (1L << 31)) return -2;   // unsigned grid-stride loops never wrap
  if (dtype == CMHAR_BF16)
    bn_bwd_launch<bf16>(M, C, x, y, dy, w, nullptr, smean, srstd, dx, dres, dw, db, training, relu, ws, stream);
  else if (dtype == CMHAR_F32)
    bn_bwd_launch<float>(M, C, x, y, dy, w, nullptr, smean, srstd, dx, dres, dw, db, training, relu, ws, stream);
  else return -1;
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_bn_cl_bwd_nores(int dtype, long M, int C, const void* x, const void* dy, const float* w,
                                     const float* b, const float* smean, const float* srstd, void* dx, float* dw,
                                     float* db, int training, int relu, float* ws, hipStream_t stream) {
  if (M <= 0 || !bn_channels_ok(C) || !ws || !dw || !db || relu < 0 || relu > 2 || (relu && !b)) return -1;
  if (M >= (1L << 31) || M * C / 8 >= (1L << 31)) return -2;   // unsigned grid-stride loops never wrap
  if (dtype == CMHAR_BF16)
    bn_bwd_launch<bf16>(M, C, x, nullptr, dy, w, b, smean, srstd, dx, nullptr, dw, db, training, relu, ws, stream);
  else if (dtype == CMHAR_F32)
    bn_bwd_launch<float>(M, C, x, nullptr, dy, w, b, smean, srstd, dx, nullptr, dw, db, training, relu, ws, stream);
  else return -1;
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_avgpool_cl(int dtype, int N, long S, int C, const void* x, float* out, hipStream_t stream) {
  if (N <= 0 || S <= 0 || !bn_channels_ok(C)) return -1;
  const int CB = C < 256 ? C : 256;
  dim3 grid(cdiv(C, CB), N);
  if (dtype == CMHAR_BF16) avgpool_cl_fwd<bf16><<<grid, 256, 0, stream>>>(N, S, C, (const bf16*)x, out);
  else if (dtype == CMHAR_F32) avgpool_cl_fwd<float><<<grid, 256, 0, stream>>>(N, S, C, (const float*)x, out);
  else return -1;
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_avgpool_cl_bwd(int dtype, int N, long S, int C, const float* dout, void* dx,
                                    hipStream_t stream) {
  if (N <= 0 || S <= 0 || C <= 0) return -1;
  const long total = (long)N * S * C;
  if (dtype == CMHAR_BF16) avgpool_cl_bwd<bf16><<<grid_for(total), 256, 0, stream>>>(total, S, C, dout, (bf16*)dx);
  else if (dtype == CMHAR_F32)
    avgpool_cl_bwd<float><<<grid_for(total), 256, 0, stream>>>(total, S, C, dout, (float*)dx);
  else return -1;
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_video_to_ndhwc(int out_dtype, int B, int T, int C, int H, int W, const float* video, void* out,
                                    hipStream_t stream) {
  if (B <= 0 || T <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
  const long total = (long)B * T * C * H * W, HW = (long)H * W;
  if (out_dtype == CMHAR_BF16)
    video_ndhwc_kernel<bf16><<<grid_for(total), 256, 0, stream>>>(total, C, HW, video, (bf16*)out);
  else if (out_dtype == CMHAR_F32)
    video_ndhwc_kernel<float><<<grid_for(total), 256, 0, stream>>>(total, C, HW, video, (float*)out);
  else return -1;
  CMHAR_CHECK_LAUNCH();
  return 0;
}
