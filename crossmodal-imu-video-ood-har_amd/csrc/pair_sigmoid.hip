// Pairwise-sigmoid (SigLIP, Zhai et al. 2023) contrastive loss with analytic gradients, tiled so that the Ba x Bb
// similarity matrix never reaches global memory.
//
//   S_ij = (a_i · b_j)·exp(t) + bias,   z_ij = +1 on the diagonal, −1 elsewhere,   w_ij = 1
//   (an off-diagonal pair of one group, ga[i] == gb[j]: same_group 0 keeps it negative, 1 ignores it (w = 0),
//   2 makes it positive)
//   loss = (1/Ba)·Σ_ij w_ij·softplus(−z_ij·S_ij),   dS_ij = −w_ij·z_ij·σ(−z_ij·S_ij)/Ba
//   da_i = e^t·Σ_j dS_ij·b_j,   db_j = e^t·Σ_i dS_ij·a_i,   gt = Σ dS_ij·(a_i·b_j)·e^t,   gbias = Σ dS_ij
//
// One kernel serves both gradient sides.  A workgroup (4 waves) owns a strip of 16 rows of the ROW operand P and
// walks the COLUMN operand Q in tiles of 64 rows; workgroups [0, nA) take P = a, Q = b (and also produce the strip's
// partial sums of loss / gt / gbias), the rest take P = b, Q = a for the strips of b that want a gradient (S is
// recomputed there: a_i·b_j commutes and k runs in the same order, so it is the same S).  Per tile:
//   1. S tile: wave w forms S[16 x 16] for tile columns 16 w .. 16 w + 15 on the f32-input MFMA (16x16x4, exact fp32,
//      k ascending) from k-slices of 64 staged in LDS ([row][k], pitch 68 floats: the 16 rows x 4 k of an operand
//      read fall on 64 distinct banks), register-prefetched one slice ahead.  Rows that are not 16-byte aligned
//      (pointer, stride or the tail of a D that is no multiple of 4) are staged with scalar loads.
//   2. z / w / softplus / σ in registers; the lane's loss, gt and gbias terms go to three running sums.
//   3. (strips that want a gradient) the dS tile passes through LDS into MFMA A-operand layout and
//      grad[16 x D] += dS[16 x 64]·Q[64 x D] runs on the MFMA: wave w owns the 16-column blocks w, w + 4, ... of D,
//      all of them in registers for the whole walk (D <= 1024: 16 blocks per wave), Q read straight from
//      global / L2 in operand layout.
// Every gradient element is therefore one fp32 chain over the Q rows in ascending order, held in one register from
// start to end; a strip is tied to the GLOBAL row index, so the result does not depend on a_off / a_cnt / b_off /
// b_cnt.  The strip partials are reduced by butterflies in a fixed order and a one-block pass adds them in a fixed
// order: no fp32 atomic anywhere, every output is a pure function of the inputs.
// With D <= 256 and enough rows that strips of 32 still fill the chip (WIDE_MIN_STRIPS) a workgroup owns two 16-row
// blocks instead of one (RB = 2): each staged slice and each Q operand load then feeds two MFMAs, which halves the
// reads of Q.  The choice is made from (Ba, Bb, D) alone.
#include "common.h"

namespace {

constexpr int CT = 64;           // Q rows per tile
constexpr int KS = 64;           // elements per k-slice
constexpr int LP = 68;           // LDS pitch of a staged slice row, floats
constexpr int DP = 68;           // LDS pitch of a dS tile row, floats
constexpr int WIDE_MIN_STRIPS = 512;   // 32-row strips from this many of them on (both sides together)
constexpr int MAX_B = 32768;
constexpr int MAX_D = 1024;

struct PairArgs {
  int Ba, Bb, D, same_group;
  const float* a;
  long lda;
  const float* b;
  long ldb;
  const long* ga;
  const long* gb;
  const float* t;
  const float* bias;
  float* da;
  int a_off, a_cnt;
  float* db;
  int b_off, b_cnt;
  float* part;                   // [3][nA]: loss, gt, gbias sums of each strip of a
  int nA, b_strip0;
  float inv;                     // 1 / Ba
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// elements k .. k + 3 of row `row` (zeros past the last row or past D)
__device__ __forceinline__ floatx4 load4(const float* base, long ld, int row, int nrows, int k, int D, bool vec) {
  floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
  if (row >= nrows) return v;
  const float* p = base + (long)row * ld + k;
  if (vec && k + 3 < D) return *(const floatx4*)p;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (k + e < D) v[e] = p[e];
  return v;
}

// NB: 16-column blocks of D per wave (D <= 64 NB); RB: 16-row blocks per strip
template <int NB, int RB>
__global__ __launch_bounds__(256) void pair_sigmoid_kernel(const PairArgs a) {
  constexpr int SR = 16 * RB;
  __shared__ __attribute__((aligned(16))) float Ps[SR * LP];
  __shared__ __attribute__((aligned(16))) float Qs[CT * LP];
  __shared__ __attribute__((aligned(16))) float dSs[SR * DP];
  __shared__ float red[3][4];

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const bool swap = (int)blockIdx.x >= a.nA;
  const int strip = swap ? a.b_strip0 + (int)blockIdx.x - a.nA : (int)blockIdx.x;
  const float* P = swap ? a.b : a.a;
  const float* Q = swap ? a.a : a.b;
  const long ldp = swap ? a.ldb : a.lda, ldq = swap ? a.lda : a.ldb;
  const int Bp = swap ? a.Bb : a.Ba, Bq = swap ? a.Ba : a.Bb;
  const long* gp = swap ? a.gb : a.ga;
  const long* gq = swap ? a.ga : a.gb;
  float* out = swap ? a.db : a.da;
  const int off = swap ? a.b_off : a.a_off, cnt = swap ? a.b_cnt : a.a_cnt;
  const int D = a.D, i0 = strip * SR;
  const bool grad = out != nullptr && i0 < off + cnt && i0 + SR > off;     // workgroup-uniform
  const bool vecP = (((uintptr_t)P & 15) == 0) && ldp % 4 == 0;
  const bool vecQ = (((uintptr_t)Q & 15) == 0) && ldq % 4 == 0;
  const bool groups = gp != nullptr;
  const int sg = a.same_group;
  const float et = expf(*a.t), bias = *a.bias, inv = a.inv;
  const int nk = (D + KS - 1) / KS, ntile = (Bq + CT - 1) / CT;

  long gi[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * rb + 4 * g + r;
      gi[rb][r] = groups && i < Bp ? gp[i] : 0;
    }

  // staging: thread t takes Q row t >> 2, elements 16 (t & 3) .. + 15, and P rows (t >> 4) + 16 rb, elements 4 (t & 15) .. + 3
  const int qrow = tid >> 2, qcol = (tid & 3) * 16, prow = tid >> 4, pcol = (tid & 15) * 4;
  floatx4 rq[4], rp[RB];
  auto load = [&](int jt, int kc) {
    const int k = kc * KS;
#pragma unroll
    for (int v = 0; v < 4; ++v) rq[v] = load4(Q, ldq, jt * CT + qrow, Bq, k + qcol + 4 * v, D, vecQ);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) rp[rb] = load4(P, ldp, i0 + 16 * rb + prow, Bp, k + pcol, D, vecP);
  };

  floatx4 acc[RB][NB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[rb][nb] = floatx4{0.f, 0.f, 0.f, 0.f};
  float l_acc = 0.f, gt_acc = 0.f, gb_acc = 0.f;

  const float* Ap = Ps + c * LP + g;                  // P row 16 rb + c, k = 4 step + g
  const float* Bp_ = Qs + (16 * w + c) * LP + g;      // Q row 16 w + c of the tile

  load(0, 0);
  for (int jt = 0; jt < ntile; ++jt) {
    floatx4 s4[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) s4[rb] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();                                // the previous slice's reads are done
#pragma unroll
      for (int v = 0; v < 4; ++v) *(floatx4*)(Qs + qrow * LP + qcol + 4 * v) = rq[v];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) *(floatx4*)(Ps + (16 * rb + prow) * LP + pcol) = rp[rb];
      __syncthreads();
      int nkc = kc + 1, njt = jt;
      if (nkc == nk) { nkc = 0; njt = jt + 1; }
      if (njt < ntile) load(njt, nkc);                // in flight during the MFMAs below
#pragma unroll
      for (int ks = 0; ks < KS / 4; ++ks) {
        const float bq = Bp_[4 * ks];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          s4[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ap[16 * rb * LP + 4 * ks], bq, s4[rb], 0, 0, 0);
      }
    }

    // C layout: s4[rb][r] = a_i·b_j for P row i0 + 16 rb + 4 g + r and Q row 64 jt + 16 w + c
    const int j = jt * CT + 16 * w + c;
    const long gj = groups && j < Bq ? gq[j] : 0;
    float ds[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * rb + 4 * g + r;
      const bool diag = i == j;
      const bool same = groups && !diag && gi[rb][r] == gj;
      const bool live = i < Bp && j < Bq && !(same && sg == 1);
      const float zz = (diag || (same && sg == 2)) ? 1.f : -1.f;
      const float dot = s4[rb][r];
      const float x = -zz * (dot * et + bias);
      const float e = expf(-fabsf(x));
      const float l = fmaxf(x, 0.f) + log1pf(e);
      const float sig = (x >= 0.f ? 1.f : e) / (1.f + e);         // σ(x) without overflow
      ds[rb][r] = live ? -zz * sig * inv : 0.f;
      l_acc += live ? l : 0.f;
      gt_acc += ds[rb][r] * dot * et;
      gb_acc += ds[rb][r];
    }

    if (grad) {
      // the previous tile's reads of dSs are at least two barriers back (nk >= 1)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dSs[(16 * rb + 4 * g + r) * DP + 16 * w + c] = ds[rb][r];
      __syncthreads();
      float af[RB][CT / 4];                           // A operand: dS[row 16 rb + c][tile column 4 ks + g]
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int ks = 0; ks < CT / 4; ++ks) af[rb][ks] = dSs[(16 * rb + c) * DP + 4 * ks + g];
#pragma unroll
      for (int nb = 0; nb < NB; nb += 2) {
        const int d0 = (w + 4 * nb) * 16 + c, d1 = d0 + 64;
        if ((w + 4 * nb) * 16 < D) {                  // wave-uniform
          float b0[CT / 4], b1[CT / 4];
#pragma unroll
          for (int ks = 0; ks < CT / 4; ++ks) {
            const int jj = jt * CT + 4 * ks + g;
            const float* q = Q + (long)jj * ldq;
            b0[ks] = jj < Bq && d0 < D ? q[d0] : 0.f;
            b1[ks] = jj < Bq && d1 < D ? q[d1] : 0.f;
          }
#pragma unroll
          for (int ks = 0; ks < CT / 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
              acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb][ks], b0[ks], acc[rb][nb], 0, 0, 0);
              acc[rb][nb + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb][ks], b1[ks], acc[rb][nb + 1], 0, 0, 0);
            }
        }
      }
    }
  }

  if (grad) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int d = (w + 4 * nb) * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * rb + 4 * g + r;
          if (d < D && i < Bp && i >= off && i < off + cnt) out[(long)(i - off) * D + d] = acc[rb][nb][r] * et;
        }
      }
  }

  if (!swap) {
    l_acc = wave_sum(l_acc);
    gt_acc = wave_sum(gt_acc);
    gb_acc = wave_sum(gb_acc);
    if (lane == 0) { red[0][w] = l_acc; red[1][w] = gt_acc; red[2][w] = gb_acc; }
    __syncthreads();
    if (tid < 3) a.part[(long)tid * a.nA + strip] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
  }
}

// one block: thread t adds strips t, t + 256, ... in ascending order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void pair_sigmoid_final(int nA, const float* __restrict__ part, float inv,
                                                          float* __restrict__ loss, float* __restrict__ gt,
                                                          float* __restrict__ gbias) {
  __shared__ float red[3][256];
  float v[3] = {0.f, 0.f, 0.f};
  for (int s = threadIdx.x; s < nA; s += 256)
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] += part[(long)q * nA + s];
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss = red[0][0] * inv;
    if (gt) *gt = red[1][0];
    if (gbias) *gbias = red[2][0];
  }
}

bool shape_ok(int Ba, int Bb, int D) {
  return Ba >= 1 && Ba <= MAX_B && Bb >= 1 && Bb <= MAX_B && D >= 1 && D <= MAX_D;
}

}  // namespace

extern "C" long cmhar_pair_sigmoid_ws(int Ba, int Bb, int D) {
  if (!shape_ok(Ba, Bb, D)) return 0;
  return 3L * cdiv(Ba, 16) * (long)sizeof(float);      // strips of 16 rows at the least
}

extern "C" int cmhar_pair_sigmoid_loss(int Ba, int Bb, int D, const float* a, long lda, const float* b, long ldb,
                                       const long* ga, const long* gb, int same_group, const float* t,
                                       const float* bias, float* loss, float* da, int a_off, int a_cnt, float* db,
                                       int b_off, int b_cnt, float* gt, float* gbias, void* ws, hipStream_t st) {
  if (!shape_ok(Ba, Bb, D) || same_group < 0 || same_group > 2) return -1;
  if (!a || !b || !t || !bias || !loss || !ws || lda < D || ldb < D || (ga == nullptr) != (gb == nullptr)) return -1;
  if (da && (a_off < 0 || a_cnt < 0 || (long)a_off + a_cnt > Ba)) return -1;
  if (db && (b_off < 0 || b_cnt < 0 || (long)b_off + b_cnt > Bb)) return -1;

  PairArgs p;
  p.Ba = Ba; p.Bb = Bb; p.D = D; p.same_group = same_group;
  p.a = a; p.lda = lda; p.b = b; p.ldb = ldb; p.ga = ga; p.gb = gb; p.t = t; p.bias = bias;
  p.da = da && a_cnt > 0 ? da : nullptr; p.a_off = a_off; p.a_cnt = a_cnt;
  p.db = db && b_cnt > 0 ? db : nullptr; p.b_off = b_off; p.b_cnt = b_cnt;
  p.part = (float*)ws;
  // strips of 32 rows halve the reads of the column operand; taken once (Ba, Bb, D) alone say that 32-row strips
  // still fill the chip, so the choice, like everything else, does not depend on the offsets / counts
  const int SR = D <= 256 && cdiv(Ba, 32) + cdiv(Bb, 32) >= WIDE_MIN_STRIPS ? 32 : 16;
  p.nA = cdiv(Ba, SR);
  p.b_strip0 = p.db ? b_off / SR : 0;
  const int nB = p.db ? (b_off + b_cnt - 1) / SR - p.b_strip0 + 1 : 0;
  p.inv = 1.f / (float)Ba;
  if (SR == 32) pair_sigmoid_kernel<4, 2><<<p.nA + nB, 256, 0, st>>>(p);
  else if (D <= 256) pair_sigmoid_kernel<4, 1><<<p.nA + nB, 256, 0, st>>>(p);
  else pair_sigmoid_kernel<16, 1><<<p.nA + nB, 256, 0, st>>>(p);
  CMHAR_CHECK_LAUNCH();
  pair_sigmoid_final<<<1, 256, 0, st>>>(p.nA, p.part, p.inv, loss, gt, gbias);
  CMHAR_CHECK_LAUNCH();
  return 0;
}
