// Class-conditional Gaussian (Mahalanobis) OOD detector: the two matmul-shaped halves, in exact fp32 on the
// f32-input MFMA (16x16x4: a k-ordered fmaf chain, one rounding per product).  16-bit features are widened to fp32 as
// they are staged, which is exact; there is no 16-bit math mode and no fp32 atomic anywhere, so each entry is a pure
// function of its inputs.
//
// cmhar_class_moments: class counts, class means and the tied scatter Σ_i (x_i − μ_{y_i})(x_i − μ_{y_i})ᵀ, in two
// passes.  Both passes are the same product Out[a][b] = Σ_i A[i][a]·B[i][b] with the ROW index as the reduction
// index, so one kernel serves both (moments_gemm_kernel):
//   pass 0  A = one-hot(labels) [N, C], B = x: the class sums.  A product with 1 is exact and adding a +0 product
//           changes nothing, so each sum is the fp32 chain over that class's rows in ascending row order; no sort
//           of the rows is needed for a fixed order.
//   pass 1  A = B = x − μ_{y_i}, formed while staging (the centred rows never exist in memory): the scatter, as an
//           upper-triangle SYRK on 128 x 128 tiles.  A[k][a]·A[k][b] commutes and both triangles of a diagonal tile
//           see the same k order, so the tile is bit-symmetric; off-diagonal tiles are written twice.
// A workgroup (4 waves; pass 1: 64 x 64 of the tile each, 4 x 4 accumulator blocks; pass 0: all class rows x 32
// columns each, skipping the 16-class blocks past C) owns one tile and one slab of rows, stages 16-row slices of both
// operands in LDS ([k][column], pitch 144 floats: the four k rows of an MFMA operand read fall on distinct banks),
// register-prefetched one slice ahead, and writes its 128 x 128 partial to the workspace.  Each pass picks its slab
// count from (N, d) alone so that tiles x slabs fills the chip.  A second small kernel adds the slabs in a fixed
// order (four quarters of the slab range, each ascending, then the quarters ascending; means: divides by the count,
// an empty class gives zeros; scatter: mirrors).  Counts are an integer histogram (integer atomics: the result does
// not depend on order).  Rows with a label outside [0, C) are staged as zeros in both passes.
//
// cmhar_class_min_dist: z = W·x per row, D[c] = Σ_j (z_j − m[c][j])², the row minimum and its first index.  A
// workgroup owns 64 rows and walks z in blocks of 64 columns: the 64 x 64 piece of z is formed on the MFMA (wave w:
// W rows 16 w .. 16 w + 15 against all 64 rows, k-slices of 32 staged as in sim_topk.hip), passed through LDS so that
// thread t holds row t & 63 of it in registers, and folded into per-(row, class) running sums: wave w serves classes
// w, w + 4, ... (the block's columns of −m are read from LDS at a wave-uniform address, i.e. broadcast; z + (−m) is
// z − m to the bit, and the add packs two columns into one v_pk_add_f32 where the compiler leaves a sub scalar).  Each
// (row, class) sum lives in one thread's register from start to end and is summed in the difference form (per block
// two packed-fp32 chains over even and odd j, their sum added to the running value, blocks in ascending order), so
// nothing depends on timing; z and the differences never reach global memory.
#include <limits.h>

#include "common.h"

namespace {

// 8 consecutive elements widened to fp32 (exact); p is 16-byte aligned
template <typename E>
__device__ __forceinline__ void load8(const E* p, float (&v)[8]) {
  if constexpr (sizeof(E) == 4) {
    const floatx4 a = *(const floatx4*)p, b = *(const floatx4*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  } else {
    typedef E __attribute__((ext_vector_type(8))) v8;
    const v8 r = *(const v8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
  }
}

__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *(floatx4*)p = floatx4{v[0], v[1], v[2], v[3]};
  *(floatx4*)(p + 4) = floatx4{v[4], v[5], v[6], v[7]};
}

// ------------------------------------------------------------------------------------------------ class moments

constexpr int TM = 128;          // tile edge
constexpr int MKS = 16;          // rows (reduction index) per staged slice
constexpr int MP = 144;          // LDS pitch of a slice row, floats
constexpr int MAX_SLABS = 256;
constexpr int TARGET_WGS = 512;  // two workgroups per CU

// Row slabs of one pass: enough workgroups (tiles x slabs) to fill the chip, at least 128 rows each
struct Slabs { int n, rps; };
Slabs slabs_for(int N, int tiles) {
  int s = TARGET_WGS / tiles;
  const int cap = cdiv(N, 128) < MAX_SLABS ? cdiv(N, 128) : MAX_SLABS;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  Slabs r;
  r.rps = cdiv(cdiv(N, s), MKS) * MKS;
  r.n = cdiv(N, r.rps);          // no empty slab
  return r;
}

struct MPlan { int nt, nts; Slabs sm, ss; long ws_floats; };

MPlan moments_plan(int N, int d) {
  MPlan p;
  p.nt = cdiv(d, TM);            // column tiles: the means pass
  p.nts = p.nt * (p.nt + 1) / 2; // upper-triangle tiles: the scatter pass
  p.sm = slabs_for(N, p.nt);
  p.ss = slabs_for(N, p.nts);
  const long a = (long)p.sm.n * p.nt, b = (long)p.ss.n * p.nts;
  p.ws_floats = (a > b ? a : b) * (TM * TM);
  return p;
}

struct MomArgs {
  int N, d, C, nt, ntiles, rps;
  const void* x;
  long ldx;
  const long* labels;
  const float* means;
  float* slabs;                  // [slab][tile][TM][TM]
};

// upper-triangle tile t -> (ta <= tb)
__device__ __forceinline__ void tri_tile(int t, int nt, int& ta, int& tb) {
  ta = 0;
  while (t >= nt - ta) { t -= nt - ta; ++ta; }
  tb = ta + t;
}

__global__ __launch_bounds__(256) void class_count_kernel(int N, int C, const long* __restrict__ labels,
                                                          int* __restrict__ counts) {
  __shared__ int h[128];
  if (threadIdx.x < 128) h[threadIdx.x] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const long l = labels[i];
    if (l >= 0 && l < C) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  if (threadIdx.x < C && h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
}

// MODE 0: slab partial of one-hot(labels)ᵀ·x (class sums); MODE 1: of (x − μ_y)ᵀ(x − μ_y), upper-triangle tiles
template <typename E, int MODE>
__global__ __launch_bounds__(256) void moments_gemm_kernel(const MomArgs a) {
  __shared__ __attribute__((aligned(16))) float As[MKS * MP];
  __shared__ __attribute__((aligned(16))) float Bs[MKS * MP];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // wave layout: MODE 1 64 x 64 of the tile (4 x 4 blocks); MODE 0 all 128 class rows x 32 columns (8 x 2 blocks),
  // so that with few classes every wave still has work
  constexpr int MI = MODE == 0 ? 8 : 4, NI = MODE == 0 ? 2 : 4;
  const int abase = MODE == 0 ? 0 : (w >> 1) * 64, bbase = MODE == 0 ? w * 32 : (w & 1) * 64;
  const int t = blockIdx.x % a.ntiles, s = blockIdx.x / a.ntiles;
  int ta = 0, tb = t;
  if (MODE == 1) tri_tile(t, a.nt, ta, tb);
  const bool two = MODE == 0 || ta != tb;      // A is staged on its own
  const int r0 = s * a.rps;
  const int r1 = r0 + a.rps < a.N ? r0 + a.rps : a.N;
  const int nsl = (r1 - r0 + MKS - 1) / MKS;
  const E* x = (const E*)a.x;

  // staging: 16 rows x 128 columns per slice and operand; thread t takes row t >> 4, columns 8 (t & 15) .. + 7
  const int srow = tid >> 4, scol = (tid & 15) * 8;
  float ra[8], rb[8];
  auto centred = [&](long i, long lab, int col, float (&v)[8]) {
    float mu[8];
    load8(x + i * a.ldx + col, v);
    load8(a.means + lab * a.d + col, mu);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] -= mu[j];
  };
  auto load = [&](int sl) {
    const long i = (long)r0 + sl * MKS + srow;
    const long lab = i < r1 ? a.labels[i] : -1;
    const bool ok = lab >= 0 && lab < a.C;
#pragma unroll
    for (int j = 0; j < 8; ++j) { ra[j] = 0.f; rb[j] = 0.f; }
    const int cb = tb * TM + scol;
    if (MODE == 0) {
      if (ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ra[j] = scol + j == lab ? 1.f : 0.f;
        if (cb < a.d) load8(x + i * a.ldx + cb, rb);
      }
    } else if (ok) {
      if (cb < a.d) centred(i, lab, cb, rb);
      const int ca = ta * TM + scol;
      if (two && ca < a.d) centred(i, lab, ca, ra);
    }
  };

  floatx4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

  const float* Ap = (two ? As : Bs) + (lane >> 4) * MP + abase + (lane & 15);
  const float* Bp = Bs + (lane >> 4) * MP + bbase + (lane & 15);

  if (nsl > 0) load(0);
  for (int sl = 0; sl < nsl; ++sl) {
    __syncthreads();                           // the previous slice's reads are done
    store8(Bs + srow * MP + scol, rb);
    if (two) store8(As + srow * MP + scol, ra);
    __syncthreads();
    if (sl + 1 < nsl) load(sl + 1);            // in flight during the MFMAs below
#pragma unroll
    for (int ks = 0; ks < MKS / 4; ++ks) {
      float bf[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) bf[ni] = Bp[ks * 4 * MP + 16 * ni];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        if (MODE == 0 && 16 * mi >= a.C) continue;                // no class there (uniform)
        const float af = Ap[ks * 4 * MP + 16 * mi];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[ni], acc[mi][ni], 0, 0, 0);
      }
    }
  }

  float* out = a.slabs + ((long)s * a.ntiles + t) * (TM * TM);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(abase + 16 * mi + 4 * (lane >> 4) + r) * TM + bbase + 16 * ni + (lane & 15)] = acc[mi][ni][r];
}

// Σ_slab p[slab * stride] for 64 elements per workgroup: thread (g, el) adds the g-th quarter of the slabs in
// ascending order, the four quarters are added in ascending order; the order is fixed by (slabs) alone.  Every
// thread of the workgroup calls it (barrier inside); the result is valid where g == 0.
__device__ __forceinline__ float slab_sum(const float* p, long stride, int slabs, bool live) {
  __shared__ float red[256];
  const int g = threadIdx.x >> 6, el = threadIdx.x & 63;
  const int per = (slabs + 3) / 4;
  const int s0 = g * per, s1 = s0 + per < slabs ? s0 + per : slabs;
  float sum = 0.f;
  if (live) {
#pragma unroll 8
    for (int s = s0; s < s1; ++s) sum += p[(long)s * stride];
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  return ((red[el] + red[64 + el]) + red[128 + el]) + red[192 + el];
}

// means[c][col] = (Σ_slab partial) / counts[c], slabs in ascending order; an empty class gives zeros
__global__ __launch_bounds__(256) void means_reduce_kernel(int d, int C, int nt, int slabs,
                                                           const float* __restrict__ part,
                                                           const int* __restrict__ counts, float* __restrict__ means) {
  const long e = (long)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < (long)C * d;
  const int c = live ? (int)(e / d) : 0, col = live ? (int)(e % d) : 0;
  const float* p = part + (long)(col / TM) * (TM * TM) + c * TM + col % TM;
  const float sum = slab_sum(p, (long)nt * (TM * TM), slabs, live);
  if (!live || threadIdx.x >= 64) return;
  const int n = counts[c];
  means[e] = n > 0 ? sum / (float)n : 0.f;
}

// scatter tile (ta, tb) = Σ_slab partial, slabs in ascending order, written to both triangles
__global__ __launch_bounds__(256) void scatter_reduce_kernel(int d, int nt, int nts, int slabs,
                                                             const float* __restrict__ part,
                                                             float* __restrict__ scatter) {
  int ta, tb;
  tri_tile(blockIdx.x, nt, ta, tb);
  const int e = blockIdx.y * 64 + (threadIdx.x & 63);
  const int ga = ta * TM + (e >> 7), gb = tb * TM + (e & 127);
  const bool live = ga < d && gb < d;
  const float* p = part + (long)blockIdx.x * (TM * TM) + e;
  const float sum = slab_sum(p, (long)nts * (TM * TM), slabs, live);
  if (!live || threadIdx.x >= 64) return;
  scatter[(long)ga * d + gb] = sum;
  if (ta != tb) scatter[(long)gb * d + ga] = sum;
}

template <typename E>
int launch_moments(MomArgs a, const MPlan& p, int* counts, float* means, float* scatter, hipStream_t st) {
  a.ntiles = p.nt;
  a.rps = p.sm.rps;
  moments_gemm_kernel<E, 0><<<p.nt * p.sm.n, 256, 0, st>>>(a);
  CMHAR_CHECK_LAUNCH();
  means_reduce_kernel<<<cdiv((long)a.C * a.d, 64), 256, 0, st>>>(a.d, a.C, p.nt, p.sm.n, a.slabs, counts, means);
  CMHAR_CHECK_LAUNCH();
  a.ntiles = p.nts;
  a.rps = p.ss.rps;
  moments_gemm_kernel<E, 1><<<p.nts * p.ss.n, 256, 0, st>>>(a);
  CMHAR_CHECK_LAUNCH();
  scatter_reduce_kernel<<<dim3(p.nts, TM * TM / 64), 256, 0, st>>>(a.d, p.nt, p.nts, p.ss.n, a.slabs, scatter);
  CMHAR_CHECK_LAUNCH();
  return 0;
}

// ----------------------------------------------------------------------------------------- class minimum distance

constexpr int BR = 64;           // rows per workgroup
constexpr int JB = 64;           // z columns per block
constexpr int KS = 32;           // elements per k-slice
constexpr int LROW = 144;        // LDS pitch of a staged k-slice row, bytes (128 + 16 pad)
constexpr int ZP = 68;           // LDS pitch of a z-tile row, floats
constexpr int STAGE_BYTES = (BR + JB) * LROW;
constexpr int ZT_BYTES = BR * ZP * 4;
constexpr int DBUF_BYTES = STAGE_BYTES > ZT_BYTES ? STAGE_BYTES : ZT_BYTES;

struct DistArgs {
  int N, d, C;
  const void* x;
  long ldx;
  const float* W;
  long ldw;
  const float* m;
  long ldm;
  float* dist2;
  int* cls;
  float* dist_all;
  long ld_all;
};

// CPT: classes per thread (wave w serves classes w, w + 4, ..., C <= 4 CPT)
template <typename E, int CPT>
__global__ __launch_bounds__(256) void class_min_dist_kernel(const DistArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sbuf[DBUF_BYTES];   // operand staging / z tile
  __shared__ __attribute__((aligned(16))) float ml[4 * CPT * JB];           // the block's columns of −m
  __shared__ float red_v[256];
  __shared__ int red_c[256];
  float* zt = (float*)sbuf;

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * BR;
  const int nk = a.d / KS, nblk = (a.d + JB - 1) / JB;
  const E* x = (const E*)a.x;

  // staging: 64 + 64 rows x 32 elements per k-slice; thread t takes row t >> 2, elements 8 (t & 3) .. + 7 of both
  const int srow = tid >> 2, scol = (tid & 3) * 8;
  float rx[8], rw[8];
  auto load = [&](int jb, int kc) {
    const int k = kc * KS + scol;
#pragma unroll
    for (int j = 0; j < 8; ++j) { rx[j] = 0.f; rw[j] = 0.f; }
    if (row0 + srow < a.N) load8(x + (row0 + srow) * a.ldx + k, rx);
    const int jr = jb * JB + srow;
    if (jr < a.d) load8(a.W + (long)jr * a.ldw + k, rw);
  };

  const unsigned char* Bx = sbuf + (lane & 15) * LROW + (lane >> 4) * 16;
  const unsigned char* Aw = sbuf + (BR + 16 * w + (lane & 15)) * LROW + (lane >> 4) * 16;

  float D[CPT];
#pragma unroll
  for (int cc = 0; cc < CPT; ++cc) D[cc] = 0.f;

  load(0, 0);
  for (int jb = 0; jb < nblk; ++jb) {
    floatx4 acc[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) acc[qi] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();                       // the previous slice's reads / the previous block's class loop are done
      store8((float*)(sbuf + srow * LROW) + scol, rx);
      store8((float*)(sbuf + (BR + srow) * LROW) + scol, rw);
      if (kc == 0) {
        for (int e = tid; e < a.C * (JB / 4); e += 256) {
          const int c = e >> 4, j4 = (e & 15) * 4, j = jb * JB + j4;
          floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
          if (j < a.d) v = -*(const floatx4*)(a.m + (long)c * a.ldm + j);   // −m: z + (−m) is z − m to the bit
          *(floatx4*)(ml + c * JB + j4) = v;
        }
      }
      __syncthreads();
      int nkc = kc + 1, njb = jb;
      if (nkc == nk) { nkc = 0; njb = jb + 1; }
      if (njb < nblk) load(njb, nkc);        // in flight during the MFMAs below
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // lane group g reads k = 16 ks + 4 g + e of its row; A and B permute k the same way
        const floatx4 af = *(const floatx4*)(Aw + ks * 64);
        floatx4 bf[4];
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) bf[qi] = *(const floatx4*)(Bx + qi * 16 * LROW + ks * 64);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int qi = 0; qi < 4; ++qi)
            acc[qi] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bf[qi][e], acc[qi], 0, 0, 0);
      }
    }

    // C layout: column (lane & 15) = row 16 qi + (lane & 15) of x, rows 4 (lane >> 4) + r = z columns 16 w + ...
    __syncthreads();                         // every wave has finished reading the staging buffer the z tile reuses
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) *(floatx4*)(zt + (16 * qi + (lane & 15)) * ZP + 16 * w + 4 * (lane >> 4)) = acc[qi];
    __syncthreads();
    // packed fp32 (v_pk_add_f32 / v_pk_fma_f32: two columns per instruction): even and odd j form two chains
    f32x2 zr[JB / 2];
#pragma unroll
    for (int j4 = 0; j4 < JB / 4; ++j4) {
      const floatx4 v = *(const floatx4*)(zt + lane * ZP + 4 * j4);
      zr[2 * j4] = f32x2{v[0], v[1]};
      zr[2 * j4 + 1] = f32x2{v[2], v[3]};
    }
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
      const int c = 4 * cc + w;
      if (c < a.C) {                         // wave-uniform
        const float* mr = ml + c * JB;
        f32x2 sblk = {0.f, 0.f};
#pragma unroll
        for (int j4 = 0; j4 < JB / 4; ++j4) {
          const floatx4 mv = *(const floatx4*)(mr + 4 * j4);
          const f32x2 d0 = zr[2 * j4] + f32x2{mv[0], mv[1]}, d1 = zr[2 * j4 + 1] + f32x2{mv[2], mv[3]};
          sblk = __builtin_elementwise_fma(d0, d0, sblk);
          sblk = __builtin_elementwise_fma(d1, d1, sblk);
        }
        D[cc] += sblk[0] + sblk[1];
      }
    }
  }

  // this thread's classes in ascending order with a strict compare: the first index of its minimum
  const long row = row0 + lane;
  float bv = INFINITY;
  int bc = INT_MAX;
#pragma unroll
  for (int cc = 0; cc < CPT; ++cc) {
    const int c = 4 * cc + w;
    if (c < a.C) {
      if (a.dist_all && row < a.N) a.dist_all[row * a.ld_all + c] = D[cc];
      if (bc == INT_MAX || D[cc] < bv) { bv = D[cc]; bc = c; }
    }
  }
  red_v[tid] = bv;
  red_c[tid] = bc;
  __syncthreads();
  if (w == 0 && row < a.N) {
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
      const float v2 = red_v[64 * ww + lane];
      const int c2 = red_c[64 * ww + lane];
      if (c2 != INT_MAX && (v2 < bv || (v2 == bv && c2 < bc))) { bv = v2; bc = c2; }
    }
    if (a.dist2) a.dist2[row] = bv;
    if (a.cls) a.cls[row] = bc;
  }
}

template <typename E>
void launch_dist(const DistArgs& a, hipStream_t st) {
  const dim3 grid(cdiv(a.N, BR));
  if (a.C <= 32) class_min_dist_kernel<E, 8><<<grid, 256, 0, st>>>(a);
  else class_min_dist_kernel<E, 32><<<grid, 256, 0, st>>>(a);
}

bool shape_ok(int N, int d, int C) { return N >= 1 && d >= 32 && d <= 1024 && d % 32 == 0 && C >= 1 && C <= 128; }

bool x_ok(int dtype, int d, const void* x, long ldx) {
  if (dtype != CMHAR_F32 && dtype != CMHAR_BF16 && dtype != CMHAR_F16) return false;
  const long ldmul = dtype == CMHAR_F32 ? 4 : 8;
  return x && ldx >= d && ldx % ldmul == 0 && ((uintptr_t)x & 15) == 0;
}

}  // namespace

extern "C" long cmhar_class_moments_ws(int N, int d, int C) {
  if (!shape_ok(N, d, C)) return 0;
  return moments_plan(N, d).ws_floats * 4;
}

extern "C" int cmhar_class_moments(int dtype, int N, int d, int C, const void* x, long ldx, const long* labels,
                                   int* counts, float* means, float* scatter, void* ws, hipStream_t st) {
  const int bad = (int)hipErrorInvalidValue;
  if (!shape_ok(N, d, C) || !x_ok(dtype, d, x, ldx)) return bad;
  if (!labels || !counts || !means || !scatter || !ws) return bad;
  if (((uintptr_t)means | (uintptr_t)ws) & 15) return bad;
  const MPlan p = moments_plan(N, d);

  hipError_t e = hipMemsetAsync(counts, 0, (size_t)C * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const int cb = cdiv(N, 256 * 8);
  class_count_kernel<<<cb < 1024 ? cb : 1024, 256, 0, st>>>(N, C, labels, counts);
  CMHAR_CHECK_LAUNCH();

  MomArgs a;
  a.N = N; a.d = d; a.C = C; a.nt = p.nt; a.ntiles = p.nt; a.rps = p.sm.rps;
  a.x = x; a.ldx = ldx; a.labels = labels; a.means = means; a.slabs = (float*)ws;
  if (dtype == CMHAR_BF16) return launch_moments<bf16>(a, p, counts, means, scatter, st);
  if (dtype == CMHAR_F16) return launch_moments<f16>(a, p, counts, means, scatter, st);
  return launch_moments<float>(a, p, counts, means, scatter, st);
}

extern "C" int cmhar_class_min_dist(int dtype, int N, int d, int C, const void* x, long ldx, const float* W, long ldw,
                                    const float* m, long ldm, float* dist2, int* cls, float* dist_all, long ld_all,
                                    hipStream_t st) {
  const int bad = (int)hipErrorInvalidValue;
  if (!shape_ok(N, d, C) || !x_ok(dtype, d, x, ldx)) return bad;
  if (!W || !m || ldw < d || ldm < d || ldw % 4 != 0 || ldm % 4 != 0) return bad;
  if (((uintptr_t)W | (uintptr_t)m) & 15) return bad;
  if (dist_all && ld_all < C) return bad;

  DistArgs a;
  a.N = N; a.d = d; a.C = C;
  a.x = x; a.ldx = ldx; a.W = W; a.ldw = ldw; a.m = m; a.ldm = ldm;
  a.dist2 = dist2; a.cls = cls; a.dist_all = dist_all; a.ld_all = ld_all;
  if (dtype == CMHAR_BF16) launch_dist<bf16>(a, st);
  else if (dtype == CMHAR_F16) launch_dist<f16>(a, st);
  else launch_dist<float>(a, st);
  CMHAR_CHECK_LAUNCH();
  return 0;
}
