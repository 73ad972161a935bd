// Fused similarity top-k: for nq query rows, the k largest dot products against an nb-row bank with their indices
// (k-NN OOD scores, cross-modal retrieval recall@k).  The nq x nb score matrix never exists: every 128 x 64 tile of
// it is formed on the matrix cores and reduced to the per-query running top-k before it leaves the CU.
//
// Tiling.  A workgroup (4 waves) owns 64 queries and one range of the bank, which it walks in ascending index order
// in chunks of 128 rows.  Both operands are staged through LDS in 128-byte k-slices (64 16-bit / 32 fp32 elements,
// rows padded to 144 B so the 16 rows of a ds_read_b128 fall on distinct banks), register-prefetched one slice
// ahead.  The product is S^T: bank rows are the MFMA's A operand and queries its B operand, so in the C layout
// (col = lane & 15, row = 4 (lane >> 4) + reg) a lane owns ONE query per 16 x 16 block and the threshold test is a
// per-lane scalar compare.  Wave w holds bank rows [32 w, 32 w + 32) x all 64 queries: 2 x 4 accumulator blocks.
// 16-bit operands use the 16x16x32 MFMA (mma16<E>); fp32 uses the exact-f32 16x16x4 MFMA, each lane reading four
// consecutive k of its row with one ds_read_b128 and feeding them to four MFMAs (A and B permute k the same way, and
// a dot product does not care).
//
// Selection.  Each query keeps a sorted k-list in LDS and its k-th value (the threshold) in a lane register.  After
// a chunk's k loop a lane compares the maximum of each accumulator's four scores with the threshold; only a wave
// that has a hit looks closer: scores that beat the threshold (strictly), lie inside the bank and are not the
// query's own row go into a 64 x 128 score tile in LDS (it reuses the staging buffer) and set their bit in a
// per-query 128-bit mask.  If any wave had a hit, each wave then serves 16 queries: it holds the query's list one
// entry per lane and the query's 128 tile slots two per lane, walks the mask's bits in ascending bank index, and
// inserts every score that still beats the threshold (v_readlane for the candidate and the new threshold, a ballot
// for the position, a DPP shift by one lane: no LDS round trip per candidate).  Candidates arrive in ascending
// index and the test is a strict >, so equal scores stay ordered by ascending bank index and the list is a pure
// function of the inputs: nothing depends on which wave got where first.
//
// Splits.  The grid is (query tiles) x (bank ranges).  The range count comes from (nq, nb, k) so that a small query
// set against a large bank still fills the chip, and never exceeds what is resident at once (sim_topk_plan);
// consecutive logical workgroups walk the SAME bank range for different query tiles, and xcd_remap keeps them on
// one XCD, so the range (the large operand) is fetched into one L2 and re-read there.  With one range the kernel
// writes vals / idx; otherwise it writes its sorted list to the workspace and a second kernel (one wave per query)
// merges the lists in range order with the same insert.
#include <limits.h>

#include "common.h"

namespace {

constexpr int BQ = 64;      // queries per workgroup
constexpr int BB = 128;     // bank rows per chunk
constexpr int KBYTES = 128; // bytes of one k-slice of a row
constexpr int LROW = 144;   // LDS row pitch of a k-slice (128 + 16 B pad)
constexpr int STAGE_BYTES = (BQ + BB) * LROW;
constexpr int TILE_BYTES = BQ * BB * 4;
constexpr int SBUF_BYTES = STAGE_BYTES > TILE_BYTES ? STAGE_BYTES : TILE_BYTES;
constexpr int NUM_CUS = 256;
constexpr int MIN_CHUNKS = 8;         // a range shorter than this pays more for its list start-up than it wins

// workgroups one CU holds at once: LDS (16 / 32 / 64-entry lists: 42 / 50 / 66 KB) and the register budget the
// kernel is compiled for
constexpr int resident_per_cu(int k) { return k <= 32 ? 3 : 2; }

struct Plan { int qtiles, nchunks, cps, splits; };

// As many bank ranges as keep every workgroup resident at once (a grid one workgroup over that runs a second,
// nearly empty round), each at least MIN_CHUNKS chunks long; every range restarts its lists from nothing, so more
// ranges than that only add insertions.
Plan sim_topk_plan(int nq, int nb, int k) {
  Plan p;
  p.qtiles = cdiv(nq, BQ);
  p.nchunks = cdiv(nb, BB);
  int s = NUM_CUS * resident_per_cu(k) / p.qtiles;
  const int cap = p.nchunks / MIN_CHUNKS;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  p.cps = cdiv(p.nchunks, s);
  p.splits = cdiv(p.nchunks, p.cps);     // no empty range
  return p;
}

struct Args {
  int nq, nb, k, rowbytes;
  const unsigned char* q;
  long ldq;                  // bytes
  const unsigned char* bank;
  long ldb;                  // bytes
  long self_offset;
  int qtiles, cps, nchunks, splits;
  float* vals;               // [nq, k] (splits == 1) or [nq, splits, k]
  int* idx;
};

// lane l's copy of lane l - 1's x (lane 0 keeps its own): DPP wave_shr:1, no LDS crossbar trip
__device__ __forceinline__ int shr1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }

// (s, j) into the descending list held one entry per lane (lanes >= k idle at -inf).  The caller has checked
// s > list[k - 1]; j is larger than every index already in the list, so the new entry goes behind its equals.
__device__ __forceinline__ void list_insert(float& v, int& ix, float s, int j, int lane, int k) {
  const int p = __popcll(__ballot(v >= s));
  const float uv = __builtin_bit_cast(float, shr1(__builtin_bit_cast(int, v)));
  const int ui = shr1(ix);
  if (lane == p) { v = s; ix = j; }
  else if (lane > p) { v = uv; ix = ui; }
  if (lane >= k) { v = -INFINITY; ix = INT_MAX; }
}

// lane `l`'s (wave-uniform l) value of x, as a scalar
__device__ __forceinline__ float lane_f(float x, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}

template <typename E, int KMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KMAX <= 32 ? 3 : 2)))   // = resident_per_cu
void sim_topk_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char sbuf[SBUF_BYTES];   // operand staging / score tile
  __shared__ float lv[BQ * KMAX];
  __shared__ int li[BQ * KMAX];
  __shared__ unsigned mask[BQ * 4];
  __shared__ float thr_s[BQ];
  float* tile = (float*)sbuf;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int sp = lin / a.qtiles, qt = lin % a.qtiles;
  const int q0 = qt * BQ;
  const int c0 = sp * a.cps, c1 = min(c0 + a.cps, a.nchunks);
  const int k = a.k;
  const int nk = (a.rowbytes + KBYTES - 1) / KBYTES;

  for (int e = tid; e < BQ * KMAX; e += 256) { lv[e] = -INFINITY; li[e] = INT_MAX; }
  mask[tid] = 0;                                                             // BQ * 4 == 256
  if (tid < BQ) thr_s[tid] = q0 + tid < a.nq ? -INFINITY : INFINITY;         // padded queries never take a score

  // this lane's queries (one per 16-column block): threshold and excluded bank row
  float thr[4];
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) thr[qi] = q0 + 16 * qi + (lane & 15) < a.nq ? -INFINITY : INFINITY;
  const long self0 = a.self_offset >= 0 ? a.self_offset + q0 + (lane & 15) : LONG_MIN;   // of block 0; +16 per block

  // staging: 192 rows x 8 16-B slots per k-slice; thread t takes slots t + 256 i (i < 2: queries, i >= 2: bank)
  const int srow = tid >> 3, scol = (tid & 7) * 16;
  uint4_t rq[2], rb[4];
  auto load = [&](int c, int kc) {
    const long kb = (long)kc * KBYTES + scol;
    const bool kin = kb < a.rowbytes;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = q0 + srow + 32 * i;
      rq[i] = uint4_t{0, 0, 0, 0};
      if (kin && r < a.nq) rq[i] = *(const uint4_t*)(a.q + (long)r * a.ldq + kb);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long r = (long)c * BB + srow + 32 * i;
      rb[i] = uint4_t{0, 0, 0, 0};
      if (kin && r < a.nb) rb[i] = *(const uint4_t*)(a.bank + r * a.ldb + kb);
    }
  };

  const unsigned char* Bq = sbuf + (lane & 15) * LROW + (lane >> 4) * 16;
  const unsigned char* Ab = sbuf + (BQ + 32 * w + (lane & 15)) * LROW + (lane >> 4) * 16;

  if (c0 < c1) load(c0, 0);
  for (int c = c0; c < c1; ++c) {
    floatx4 acc[2][4];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) acc[bi][qi] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int kc = 0; kc < nk; ++kc) {
      __syncthreads();                       // the previous slice's reads / the previous chunk's merge are done
#pragma unroll
      for (int i = 0; i < 2; ++i) *(uint4_t*)(sbuf + (srow + 32 * i) * LROW + scol) = rq[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4_t*)(sbuf + (BQ + srow + 32 * i) * LROW + scol) = rb[i];
      __syncthreads();
      int nkc = kc + 1, nc = c;
      if (nkc == nk) { nkc = 0; nc = c + 1; }
      if (nc < c1) load(nc, nkc);            // in flight during the MFMAs below
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if constexpr (sizeof(E) == 2) {
          bf16x8 af[2], bf[4];
#pragma unroll
          for (int bi = 0; bi < 2; ++bi) af[bi] = *(const bf16x8*)(Ab + bi * 16 * LROW + ks * 64);
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) bf[qi] = *(const bf16x8*)(Bq + qi * 16 * LROW + ks * 64);
#pragma unroll
          for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) acc[bi][qi] = mma16<E>(af[bi], bf[qi], acc[bi][qi]);
        } else {
          floatx4 af[2], bf[4];
#pragma unroll
          for (int bi = 0; bi < 2; ++bi) af[bi] = *(const floatx4*)(Ab + bi * 16 * LROW + ks * 64);
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) bf[qi] = *(const floatx4*)(Bq + qi * 16 * LROW + ks * 64);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
              for (int qi = 0; qi < 4; ++qi)
                acc[bi][qi] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[bi][e], bf[qi][e], acc[bi][qi], 0, 0, 0);
        }
      }
    }

    // ---- selection ----
    bool hit = false;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const floatx4 s = acc[bi][qi];
        hit |= fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])) > thr[qi];
      }
    const bool whit = __any(hit);
    __syncthreads();                         // every wave has finished reading the staging buffer the tile reuses
    if (whit) {
      const long cbase = (long)c * BB;
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int qi = 0; qi < 4; ++qi)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int loc = 32 * w + 16 * bi + 4 * (lane >> 4) + r;
            const long j = cbase + loc;
            const float s = acc[bi][qi][r];
            if (s > thr[qi] && j < a.nb && j - 16 * qi != self0) {
              const int ql = 16 * qi + (lane & 15);
              tile[ql * BB + loc] = s;
              atomicOr(&mask[ql * 4 + (loc >> 5)], 1u << (loc & 31));
            }
          }
    }
    if (__syncthreads_or(whit)) {
      // wave w serves queries w + 4 i: one read fetches their 16 x 4 mask words (query i in lanes 4 i .. 4 i + 3)
      const unsigned mw = mask[(w + 4 * (lane >> 2)) * 4 + (lane & 3)];
      unsigned long long nz = __ballot(mw != 0);
      while (nz) {
        const int i = __builtin_ctzll(nz) >> 2;
        nz &= ~(0xFull << (4 * i));
        const int ql = w + 4 * i;
        float v = lane < k ? lv[ql * KMAX + lane] : -INFINITY;
        int ix = lane < k ? li[ql * KMAX + lane] : INT_MAX;
        // the query's 128 tile slots, two per lane (slots without a mask bit hold stale values nobody looks at)
        const float cand[2] = {tile[ql * BB + lane], tile[ql * BB + 64 + lane]};
        float t = lane_f(v, k - 1);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          unsigned mm = __builtin_amdgcn_readlane(mw, 4 * i + x);
          while (mm) {
            const int b = __builtin_ctz(mm);
            mm &= mm - 1;
            const float s = lane_f(cand[x >> 1], 32 * (x & 1) + b);
            if (s > t) {
              list_insert(v, ix, s, (int)((long)c * BB + 32 * x + b), lane, k);
              t = lane_f(v, k - 1);
            }
          }
        }
        if (lane < k) { lv[ql * KMAX + lane] = v; li[ql * KMAX + lane] = ix; }
        if (lane < 4) mask[ql * 4 + lane] = 0;
        if (lane == 0) thr_s[ql] = t;
      }
      __syncthreads();
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) thr[qi] = thr_s[16 * qi + (lane & 15)];
    }
  }

  __syncthreads();
  for (int e = tid; e < BQ * k; e += 256) {
    const int ql = e / k, r = e % k;
    const int qg = q0 + ql;
    if (qg < a.nq) {
      const long o = ((long)qg * a.splits + sp) * k + r;
      a.vals[o] = lv[ql * KMAX + r];
      a.idx[o] = li[ql * KMAX + r];
    }
  }
}

// One wave per query: the `splits` sorted partial lists, in bank-range order, through the same insert.
__global__ __launch_bounds__(256) void sim_topk_merge_kernel(int nq, int k, int splits, const float* __restrict__ wv,
                                                             const int* __restrict__ wi, float* __restrict__ vals,
                                                             int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;                                    // wave-uniform
  float v = -INFINITY, t = -INFINITY;
  int ix = INT_MAX;
  for (int sp = 0; sp < splits; ++sp) {
    const long base = ((long)q * splits + sp) * k;
    const float sv = lane < k ? wv[base + lane] : -INFINITY;
    const int si = lane < k ? wi[base + lane] : INT_MAX;
    for (int e = 0; e < k; ++e) {
      const float s = lane_f(sv, e);
      if (!(s > t)) break;                                // the rest of this list is no larger
      list_insert(v, ix, s, __builtin_amdgcn_readlane(si, e), lane, k);
      t = lane_f(v, k - 1);
    }
  }
  if (lane < k) { vals[(long)q * k + lane] = v; idx[(long)q * k + lane] = ix; }
}

template <typename E>
void launch(const Args& a, hipStream_t st) {
  const dim3 grid(a.qtiles * a.splits);
  if (a.k <= 16) sim_topk_kernel<E, 16><<<grid, 256, 0, st>>>(a);
  else if (a.k <= 32) sim_topk_kernel<E, 32><<<grid, 256, 0, st>>>(a);
  else sim_topk_kernel<E, 64><<<grid, 256, 0, st>>>(a);
}

bool shape_ok(int nq, int nb, int k) { return nq >= 1 && nb >= 1 && k >= 1 && k <= 64; }

}  // namespace

extern "C" int cmhar_sim_topk_splits(int nq, int nb, int k) {
  if (!shape_ok(nq, nb, k)) return 0;
  return sim_topk_plan(nq, nb, k).splits;
}

extern "C" long cmhar_sim_topk_ws(int nq, int nb, int k) {
  if (!shape_ok(nq, nb, k)) return 0;
  const int s = sim_topk_plan(nq, nb, k).splits;
  return s > 1 ? (long)nq * s * k * 8 : 0;
}

extern "C" int cmhar_sim_topk(int dtype, int nq, int nb, int d, int k, const void* q, long ldq, const void* bank,
                              long ldb, long self_offset, float* vals, int* idx, void* ws, hipStream_t st) {
  const int bad = (int)hipErrorInvalidValue;
  if (dtype != CMHAR_F32 && dtype != CMHAR_BF16 && dtype != CMHAR_F16) return bad;
  if (!shape_ok(nq, nb, k) || d < 32 || d > 1024 || d % 32 != 0 || self_offset < -1) return bad;
  if ((long)k > (long)nb - (self_offset >= 0 ? 1 : 0)) return bad;
  const int es = dtype == CMHAR_F32 ? 4 : 2;
  const long ldm = 16 / es;
  if (!q || !bank || !vals || !idx || ldq < d || ldb < d || ldq % ldm != 0 || ldb % ldm != 0) return bad;
  if (((uintptr_t)q | (uintptr_t)bank) & 15) return bad;
  const Plan p = sim_topk_plan(nq, nb, k);
  if (p.splits > 1 && !ws) return bad;
  if ((long)p.qtiles * p.splits > INT_MAX) return bad;

  Args a;
  a.nq = nq; a.nb = nb; a.k = k; a.rowbytes = d * es;
  a.q = (const unsigned char*)q; a.ldq = ldq * es;
  a.bank = (const unsigned char*)bank; a.ldb = ldb * es;
  a.self_offset = self_offset;
  a.qtiles = p.qtiles; a.cps = p.cps; a.nchunks = p.nchunks; a.splits = p.splits;
  float* wv = (float*)ws;
  int* wi = (int*)(wv + (long)nq * p.splits * k);
  a.vals = p.splits > 1 ? wv : vals;
  a.idx = p.splits > 1 ? wi : idx;
  if (dtype == CMHAR_BF16) launch<bf16>(a, st);
  else if (dtype == CMHAR_F16) launch<f16>(a, st);
  else launch<float>(a, st);
  CMHAR_CHECK_LAUNCH();
  if (p.splits > 1) {
    sim_topk_merge_kernel<<<cdiv(nq, 4), 256, 0, st>>>(nq, k, p.splits, wv, wi, vals, idx);
    CMHAR_CHECK_LAUNCH();
  }
  return 0;
}
