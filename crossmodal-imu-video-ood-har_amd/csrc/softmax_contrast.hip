// Softmax contrastive loss (CLIP / InfoNCE, reference losses.py:57-87; with group ids the cross-modal supervised
// contrastive form) over one batch of B pairs, with analytic gradients, tiled so that the B x B similarity matrix never
// reaches global memory.
//
//   S_ij = (a_i · b_j)·exp(t),   same_ij = i != j and ids[i] == ids[j]   (all false without ids)
//   P_i = {i} ∪ {j : same_ij} for same_group 2, else {i};   n_i = |P_i|;   V_ij = not (same_group == 1 and same_ij)
//   lse_r[i] = log Σ_j V_ij e^{S_ij},   lse_c[j] = log Σ_i V_ij e^{S_ij}
//   loss = 1/(2B)·Σ_i [lse_r[i] − (1/n_i) Σ_{p∈P_i} S_ip + lse_c[i] − (1/n_i) Σ_{p∈P_i} S_pi]
//   dS_ij = 1/(2B)·[V_ij (e^{S_ij − lse_r[i]} + e^{S_ij − lse_c[j]}) − 2·[j ∈ P_i]/n_i]
//   da_i = e^t Σ_j dS_ij b_j,   db_j = e^t Σ_i dS_ij a_i,   gt = Σ_ij dS_ij S_ij
//
// Two passes of one kernel template, the tile walk of pair_sigmoid.hip: a workgroup (4 waves) owns a strip of 16 (or 32)
// rows of the ROW operand P and walks the COLUMN operand Q in tiles of 64 rows; side 0 is P = a, Q = b, side 1 is
// P = b, Q = a (a_i·b_j commutes and k runs in the same order, so both sides and both passes see the same S, to the
// bit).  Wave w forms S[16 x 16] for tile columns 16 w .. 16 w + 15 on the f32-input MFMA (16x16x4, exact fp32, k
// ascending) from k-slices of 64 staged in LDS ([row][k], pitch 68 floats: the 16 rows x 4 k of an operand read fall on
// 64 distinct banks), register-prefetched one slice ahead; rows that are not 16-byte aligned take scalar loads.
//
// Pass 1 (every strip of both sides) keeps, per row and per lane, an online softmax over the lane's columns: the
// running max m, l' = Σ e^{S−m} over every live element but the maximum itself (so l = 1 + l' and log l = log1p(l')
// keeps its precision when one pair dominates), u = Σ e^{S−m}·(S − m), and Σ_{p∈P_i} S_ip, n_i.  A masked element
// (same group under 'ignore', or a padded column past B) changes nothing, so a tile that is masked entirely leaves
// m at −∞ and nothing is ever computed from −∞ − (−∞); the first live element of a row starts its state.  The lanes'
// states are merged by butterflies, the waves' through LDS in wave order.  Per row that gives m, log l and 1/n_i
// (workspace, read by pass 2), and the row's terms of the loss, (m − pos/n) + log l, and of gt, (m − pos/n) + u/l;
// the strip's sums go to the workspace and a one-block kernel adds them in a fixed order.  Loss and gt need nothing
// else, so a call without da / db runs pass 1 only.
// Pass 2 (the strips whose gradient rows are wanted) recomputes the S tile, forms dS from the two sides' (m, log l)
// — on the diagonal as expm1 + expm1 + (2 − 2/n), which keeps e^x − 1 when the pair's probability is 1 to rounding —
// passes it through LDS into MFMA A-operand layout and accumulates grad[16 x D] += dS[16 x 64]·Q[64 x D] on the MFMA,
// wave w owning the 16-column blocks w, w + 4, ... of D in registers for the whole walk (D <= 1024: 16 blocks).
//
// Every gradient element is one fp32 chain over the Q rows in ascending order; a strip is tied to the GLOBAL row index
// and the strip height depends on (B, D) alone, so no output depends on a_off / a_cnt / b_off / b_cnt.  No fp32 atomic
// anywhere: every output is a pure function of the inputs.  Contraction is off in this file: S = dot·e^t must be the
// same rounded number wherever it is subtracted from a stored maximum.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CT = 64;           // Q rows per tile
constexpr int KS = 64;           // elements per k-slice
constexpr int LP = 68;           // LDS pitch of a staged slice row, floats
constexpr int DP = 68;           // LDS pitch of a dS tile row, floats
constexpr int WIDE_MIN_STRIPS = 512;   // 32-row strips from this many of them on (both sides together)
constexpr int MAX_B = 32768;
constexpr int MAX_D = 1024;

struct SmcArgs {
  int B, D, same_group;
  const float* a;
  long lda;
  const float* b;
  long ldb;
  const long* ids;
  const float* t;
  float* da;
  int a_off, a_cnt;
  float* db;
  int b_off, b_cnt;
  float* mx;                     // [2][B] row maximum of side 0 (rows of a) / side 1 (rows of b)
  float* logl;                   // [2][B] log Σ e^{S − max}
  float* invn;                   // [B] 1 / n_i
  float* part;                   // [2 sides][2: loss, gt][nS] strip sums of pass 1
  int nS;                        // pass 1: strips per side
  int s0[2], ns0;                // pass 2: first strip of each side, strips of side 0 in the grid
  float inv;                     // 1 / (2 B)
};

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

// online-softmax state of the live elements seen so far: m their maximum (−∞: none yet), lp = Σ e^{S−m} without the
// maximum's own 1, u = Σ e^{S−m}·(S − m)
struct Soft {
  float m, lp, u;
};

__device__ __forceinline__ void soft_add(Soft& s, float x) {
  const bool first = s.m == -INFINITY;
  const float d = first ? 0.f : x - s.m;
  const float e = expf(-fabsf(d));
  const float l = first ? 0.f : s.lp + 1.f;
  if (first || d > 0.f) {                             // a new maximum: the old one joins the others
    s.lp = l * e;
    s.u = e * (s.u - l * d);
    s.m = x;
  } else {
    s.lp += e;
    s.u += e * d;
  }
}

// x + y, where the state with the larger maximum keeps its terms as they are
__device__ __forceinline__ Soft soft_merge(const Soft& x, const Soft& y) {
  const bool xs = x.m >= y.m;
  const Soft& hi = xs ? x : y;
  const Soft& lo = xs ? y : x;
  const bool none = lo.m == -INFINITY;
  const float d = none ? 0.f : lo.m - hi.m;
  const float e = none ? 0.f : expf(d);
  const float l = none ? 0.f : lo.lp + 1.f;
  return Soft{hi.m, hi.lp + l * e, hi.u + e * (lo.u + l * d)};
}

// NB: 16-column blocks of D per wave (D <= 64 NB; pass 2 only); RB: 16-row blocks per strip; PASS: 1 or 2
template <int NB, int RB, int PASS>
__global__ __launch_bounds__(256) void softmax_contrast_kernel(const SmcArgs a) {
  constexpr int SR = 16 * RB;
  __shared__ __attribute__((aligned(16))) float Ps[SR * LP];
  __shared__ __attribute__((aligned(16))) float Qs[CT * LP];
  __shared__ __attribute__((aligned(16))) float Xs[PASS == 2 ? SR * DP : 4 * SR * 5];   // dS tile / wave states

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int split = PASS == 1 ? a.nS : a.ns0;
  const int side = (int)blockIdx.x >= split ? 1 : 0;
  const int strip = (PASS == 1 ? 0 : a.s0[side]) + (int)blockIdx.x - side * split;
  const float* P = side ? a.b : a.a;
  const float* Q = side ? a.a : a.b;
  const long ldp = side ? a.ldb : a.lda, ldq = side ? a.lda : a.ldb;
  const int B = a.B, D = a.D, i0 = strip * SR;
  const bool vecP = (((uintptr_t)P & 15) == 0) && ldp % 4 == 0;
  const bool vecQ = (((uintptr_t)Q & 15) == 0) && ldq % 4 == 0;
  const long* ids = a.ids;
  const bool groups = ids != nullptr;
  const int sg = a.same_group;
  const float et = expf(*a.t), inv = a.inv;
  const int nk = (D + KS - 1) / KS, ntile = (B + CT - 1) / CT;

  long gi[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * rb + 4 * g + r;
      gi[rb][r] = groups && i < B ? ids[i] : 0;
    }

  // staging: thread t takes Q row t >> 2, elements 16 (t & 3) .. + 15, and P rows (t >> 4) + 16 rb, elements 4 (t & 15) .. + 3
  const int qrow = tid >> 2, qcol = (tid & 3) * 16, prow = tid >> 4, pcol = (tid & 15) * 4;
  floatx4 rq[4], rp[RB];
  auto load = [&](int jt, int kc) {
    const int k = kc * KS;
#pragma unroll
    for (int v = 0; v < 4; ++v) rq[v] = load4(Q, ldq, jt * CT + qrow, B, k + qcol + 4 * v, D, vecQ);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) rp[rb] = load4(P, ldp, i0 + 16 * rb + prow, B, k + pcol, D, vecP);
  };

  // pass 1: the lane's running states; pass 2: the rows' statistics and the gradient accumulators
  Soft st[RB][4];
  float ps[RB][4];
  int np[RB][4];
  float mP[RB][4], lP[RB][4], nP[RB][4];
  floatx4 acc[RB][NB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      st[rb][r] = Soft{-INFINITY, 0.f, 0.f};
      ps[rb][r] = 0.f;
      np[rb][r] = 0;
      mP[rb][r] = lP[rb][r] = nP[rb][r] = 0.f;
      if constexpr (PASS == 2) {
        const int i = i0 + 16 * rb + 4 * g + r;
        if (i < B) {
          mP[rb][r] = a.mx[(long)side * B + i];
          lP[rb][r] = a.logl[(long)side * B + i];
          nP[rb][r] = a.invn[i];
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[rb][nb] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  const float* mQ = a.mx + (long)(1 - side) * B;
  const float* lQ = a.logl + (long)(1 - side) * B;

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
    const long gj = groups && j < B ? ids[j] : 0;
    if constexpr (PASS == 1) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * rb + 4 * g + r;
          const bool inb = i < B && j < B, diag = i == j;
          const bool same = groups && !diag && gi[rb][r] == gj;
          const float s = s4[rb][r] * et;
          if (inb && (diag || (same && sg == 2))) { ps[rb][r] += s; np[rb][r] += 1; }
          if (inb && !(same && sg == 1)) soft_add(st[rb][r], s);
        }
    } else {
      float mq = 0.f, lq = 0.f;
      if (j < B) { mq = mQ[j]; lq = lQ[j]; }
      // wave-uniform: the wave's 16 columns of this tile cross the strip's rows, so the diagonal is among them
      const int j0 = jt * CT + 16 * w;
      const bool has_diag = j0 < i0 + SR && j0 + 16 > i0;
      float ds[RB][4];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * rb + 4 * g + r;
          const bool inb = i < B && j < B, diag = i == j;
          const bool same = groups && !diag && gi[rb][r] == gj;
          const bool live = inb && !(same && sg == 1);
          const bool pos = inb && (diag || (same && sg == 2));
          const float s = s4[rb][r] * et;
          const float xr = (s - mP[rb][r]) - lP[rb][r], xc = (s - mq) - lq;
          const float p = live ? expf(xr) + expf(xc) : 0.f;
          ds[rb][r] = (p - (pos ? 2.f * nP[rb][r] : 0.f)) * inv;
        }
      if (has_diag) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + 16 * rb + 4 * g + r;
            if (i == j && i < B) {
              const float s = s4[rb][r] * et;
              const float xr = (s - mP[rb][r]) - lP[rb][r], xc = (s - mq) - lq;
              ds[rb][r] = ((expm1f(xr) + expm1f(xc)) + (2.f - 2.f * nP[rb][r])) * inv;
            }
          }
      }

      // the previous tile's reads of Xs are at least two barriers back (nk >= 1)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(16 * rb + 4 * g + r) * DP + 16 * w + c] = ds[rb][r];
      __syncthreads();
      float af[RB][CT / 4];                           // A operand: dS[row 16 rb + c][tile column 4 ks + g]
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int ks = 0; ks < CT / 4; ++ks) af[rb][ks] = Xs[(16 * rb + c) * DP + 4 * ks + g];
#pragma unroll
      for (int nb = 0; nb < NB; nb += 2) {
        const int d0 = (w + 4 * nb) * 16 + c, d1 = d0 + 64;
        if ((w + 4 * nb) * 16 < D) {                  // wave-uniform
          float b0[CT / 4], b1[CT / 4];
#pragma unroll
          for (int ks = 0; ks < CT / 4; ++ks) {
            const int jj = jt * CT + 4 * ks + g;
            const float* q = Q + (long)jj * ldq;
            b0[ks] = jj < B && d0 < D ? q[d0] : 0.f;
            b1[ks] = jj < B && d1 < D ? q[d1] : 0.f;
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

  if constexpr (PASS == 2) {
    float* out = side ? a.db : a.da;
    const int off = side ? a.b_off : a.a_off, cnt = side ? a.b_cnt : a.a_cnt;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int d = (w + 4 * nb) * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * rb + 4 * g + r;
          if (d < D && i < B && i >= off && i < off + cnt) out[(long)(i - off) * D + d] = acc[rb][nb][r] * et;
        }
      }
  } else {
    // the 16 lanes of a row (butterfly over c), then the 4 waves in order, then the strip's rows in order
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Soft s = st[rb][r];
        float p = ps[rb][r];
        int n = np[rb][r];
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
          const Soft y{__shfl_xor(s.m, o), __shfl_xor(s.lp, o), __shfl_xor(s.u, o)};
          s = soft_merge(s, y);
          p += __shfl_xor(p, o);
          n += __shfl_xor(n, o);
        }
        if (c == 0) {
          float* x = Xs + (w * SR + 16 * rb + 4 * g + r) * 5;
          x[0] = s.m; x[1] = s.lp; x[2] = s.u; x[3] = p; x[4] = (float)n;
        }
      }
    __syncthreads();
    float row_l = 0.f, row_g = 0.f;
    if (tid < SR) {
      const float* x = Xs + tid * 5;
      Soft s{x[0], x[1], x[2]};
      float p = x[3], n = x[4];
#pragma unroll
      for (int ww = 1; ww < 4; ++ww) {
        const float* y = Xs + (ww * SR + tid) * 5;
        s = soft_merge(s, Soft{y[0], y[1], y[2]});
        p += y[3];
        n += y[4];
      }
      const int i = i0 + tid;
      if (i < B) {                                    // the diagonal is always live: m is finite, n >= 1
        const float ll = log1pf(s.lp), base = s.m - p / n;
        a.mx[(long)side * B + i] = s.m;
        a.logl[(long)side * B + i] = ll;
        if (side == 0) a.invn[i] = 1.f / n;
        row_l = base + ll;
        row_g = base + s.u / (s.lp + 1.f);
      }
    }
    __syncthreads();
    if (tid < SR) { Xs[tid] = row_l; Xs[SR + tid] = row_g; }
    __syncthreads();
    if (tid < 2) {
      float v = 0.f;
      for (int r = 0; r < SR; ++r) v += Xs[tid * SR + r];
      a.part[((long)side * 2 + tid) * a.nS + strip] = v;
    }
  }
}

// one block: thread t adds strips t, t + 256, ... in ascending order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void softmax_contrast_final(int nS, const float* __restrict__ part, float inv,
                                                              float* __restrict__ loss, float* __restrict__ gt) {
  __shared__ float red[4][256];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = threadIdx.x; s < nS; s += 256)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += part[(long)q * nS + s];
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {                             // part: [side][loss, gt]
    *loss = (red[0][0] + red[2][0]) * inv;
    if (gt) *gt = (red[1][0] + red[3][0]) * inv;
  }
}

bool shape_ok(int B, int D) { return B >= 1 && B <= MAX_B && D >= 1 && D <= MAX_D; }

// floats: mx [2][B], logl [2][B], invn [B], part [4][strips of 16 rows at the least]
long ws_floats(int B) { return 5L * B + 4L * cdiv(B, 16); }

}  // namespace

extern "C" long cmhar_softmax_contrast_ws(int B, int D) {
  if (!shape_ok(B, D)) return 0;
  return ws_floats(B) * (long)sizeof(float);
}

extern "C" int cmhar_softmax_contrast_loss(int B, int D, const float* a, long lda, const float* b, long ldb,
                                           const long* ids, int same_group, const float* t, float* loss, float* da,
                                           int a_off, int a_cnt, float* db, int b_off, int b_cnt, float* gt, void* ws,
                                           hipStream_t st) {
  if (!shape_ok(B, D) || same_group < 0 || same_group > 2) return -1;
  if (!a || !b || !t || !loss || !ws || lda < D || ldb < D) return -1;
  if (da && (a_off < 0 || a_cnt < 0 || (long)a_off + a_cnt > B)) return -1;
  if (db && (b_off < 0 || b_cnt < 0 || (long)b_off + b_cnt > B)) return -1;

  SmcArgs p;
  p.B = B; p.D = D; p.same_group = same_group;
  p.a = a; p.lda = lda; p.b = b; p.ldb = ldb; p.ids = ids; p.t = t;
  p.da = da && a_cnt > 0 ? da : nullptr; p.a_off = a_off; p.a_cnt = a_cnt;
  p.db = db && b_cnt > 0 ? db : nullptr; p.b_off = b_off; p.b_cnt = b_cnt;
  float* f = (float*)ws;
  p.mx = f; p.logl = f + 2L * B; p.invn = f + 4L * B; p.part = f + 5L * B;
  p.inv = 0.5f / (float)B;
  p.s0[0] = p.s0[1] = p.ns0 = 0;
  // strips of 32 rows halve the reads of the column operand; taken once B alone says that 32-row strips still fill
  // the chip (pass 2: and D <= 256, where the accumulators of two row blocks fit), never from the offsets / counts
  const bool wide = 2 * cdiv(B, 32) >= WIDE_MIN_STRIPS;
  if (wide) {
    p.nS = cdiv(B, 32);
    softmax_contrast_kernel<1, 2, 1><<<2 * p.nS, 256, 0, st>>>(p);
  } else {
    p.nS = cdiv(B, 16);
    softmax_contrast_kernel<1, 1, 1><<<2 * p.nS, 256, 0, st>>>(p);
  }
  CMHAR_CHECK_LAUNCH();
  softmax_contrast_final<<<1, 256, 0, st>>>(p.nS, p.part, p.inv, loss, gt);
  CMHAR_CHECK_LAUNCH();
  if (!p.da && !p.db) return 0;

  const int SR = wide && D <= 256 ? 32 : 16;
  int n[2] = {0, 0};
  if (p.da) { p.s0[0] = a_off / SR; n[0] = (a_off + a_cnt - 1) / SR - p.s0[0] + 1; }
  if (p.db) { p.s0[1] = b_off / SR; n[1] = (b_off + b_cnt - 1) / SR - p.s0[1] + 1; }
  p.ns0 = n[0];
  if (SR == 32) softmax_contrast_kernel<4, 2, 2><<<n[0] + n[1], 256, 0, st>>>(p);
  else if (D <= 256) softmax_contrast_kernel<4, 1, 2><<<n[0] + n[1], 256, 0, st>>>(p);
  else softmax_contrast_kernel<16, 1, 2><<<n[0] + n[1], 256, 0, st>>>(p);
  CMHAR_CHECK_LAUNCH();
  return 0;
}
