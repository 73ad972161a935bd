// Masked-token encoding (FLIP-style pretraining on VideoMAE tube masks): the patch matrix and the position rows of the
// KEPT tokens only.  Masked patches of the fp32 video are never read.
#include "common.h"

namespace {

__device__ __forceinline__ int clamp_row(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// tubelet_im2col_kernel (misc.hip) with the token taken from keep_idx [B, Lkeep]: output row b·Lkeep + j is the row
// b·L + keep_idx[b][j] of the full patch matrix — same column order (c, dt, dy, dx), same 8-wide dx groups, same
// rounding (modeling_videomae.py:109-122: embeddings[~bool_masked_pos], taken before the projection instead of after).
// Every index is clamped into [0, L): a bad index reads a wrong patch, never outside the video.
template <typename TO>
__global__ void tubelet_im2col_gather_kernel(int B, int T, int C, int H, int W, int tub, int P,
                                             const float* __restrict__ v, const int* __restrict__ keep, int Lkeep,
                                             TO* __restrict__ out) {
  const int Tp = T / tub, Hp = H / P, Wp = W / P;
  const int L = Tp * Hp * Wp;
  const int K = C * tub * P * P;
  const int groups = P / 8;                  // 8 consecutive dx per thread
  const long total = (long)B * Lkeep * C * tub * P * groups;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  long r = idx;
  const int gx = r % groups; r /= groups;
  const int dy = r % P; r /= P;
  const int dt = r % tub; r /= tub;
  const int c = r % C; r /= C;                // r = output row b·Lkeep + j
  const int b = r / Lkeep;
  const int tok = clamp_row(keep[r], L);
  const int wp = tok % Wp, hp = (tok / Wp) % Hp, tp = tok / (Wp * Hp);
  const float* src = v + ((((long)b * T + tp * tub + dt) * C + c) * H + hp * P + dy) * W + wp * P + gx * 8;
  TO* dst = out + r * K + ((c * tub + dt) * P + dy) * P + gx * 8;
  const floatx4 x0 = *(const floatx4*)src, x1 = *(const floatx4*)(src + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { dst[j] = from_f<TO>(x0[j]); dst[4 + j] = from_f<TO>(x1[j]); }
}

// out[m, :] = table[clamp(idx[m]), :] — one thread per V consecutive floats of a row (V = 4: 16-B loads and stores).
template <int V>
__global__ void gather_rows_f32_kernel(int M, int N, const float* __restrict__ table, long ld_table, int rows_in_table,
                                       const int* __restrict__ idx, float* __restrict__ out, long ld_out) {
  const int nv = N / V;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * nv) return;
  const int m = i / nv, n = (int)(i % nv) * V;
  const float* src = table + (long)clamp_row(idx[m], rows_in_table) * ld_table + n;
  float* dst = out + (long)m * ld_out + n;
  if (V == 4) *(floatx4*)dst = *(const floatx4*)src;
  else *dst = *src;
}

}  // namespace

extern "C" int cmhar_tubelet_im2col_gather(int out_dtype, int B, int T, int C, int H, int W, int tub, int P,
                                           const float* video, const int* keep_idx, int Lkeep, void* out,
                                           hipStream_t st) {
  if (B < 1 || T < 1 || C < 1 || H < 1 || W < 1 || tub < 1 || P < 8 || Lkeep < 1) return -1;
  if (P % 8 != 0 || T % tub || H % P || W % P) return -1;
  if (!video || !keep_idx || !out) return -1;
  if (out_dtype != CMHAR_F32 && out_dtype != CMHAR_BF16 && out_dtype != CMHAR_F16) return -1;
  if ((long)(T / tub) * (H / P) * (W / P) > 0x7fffffffL || (long)B * Lkeep > 0x7fffffffL) return -1;
  const long total = (long)B * Lkeep * C * tub * P * (P / 8);
  if (total > 0x7fffffffL * 256) return -1;
  if (out_dtype == CMHAR_BF16)
    tubelet_im2col_gather_kernel<bf16><<<cdiv(total, 256), 256, 0, st>>>(B, T, C, H, W, tub, P, video, keep_idx, Lkeep,
                                                                         (bf16*)out);
  else if (out_dtype == CMHAR_F16)
    tubelet_im2col_gather_kernel<f16><<<cdiv(total, 256), 256, 0, st>>>(B, T, C, H, W, tub, P, video, keep_idx, Lkeep,
                                                                        (f16*)out);
  else
    tubelet_im2col_gather_kernel<float><<<cdiv(total, 256), 256, 0, st>>>(B, T, C, H, W, tub, P, video, keep_idx,
                                                                          Lkeep, (float*)out);
  CMHAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cmhar_gather_rows_f32(int M, int N, const float* table, long ld_table, int rows_in_table,
                                     const int* idx, float* out, long ld_out, hipStream_t st) {
  if (M < 1 || N < 1 || rows_in_table < 1 || ld_table < N || ld_out < N) return -1;
  if (!table || !idx || !out) return -1;
  const bool v4 = N % 4 == 0 && ld_table % 4 == 0 && ld_out % 4 == 0 && (uintptr_t)table % 16 == 0 &&
                  (uintptr_t)out % 16 == 0;
  const long total = (long)M * (v4 ? N / 4 : N);
  if (total > 0x7fffffffL * 256) return -1;
  if (v4)
    gather_rows_f32_kernel<4><<<cdiv(total, 256), 256, 0, st>>>(M, N, table, ld_table, rows_in_table, idx, out, ld_out);
  else
    gather_rows_f32_kernel<1><<<cdiv(total, 256), 256, 0, st>>>(M, N, table, ld_table, rows_in_table, idx, out, ld_out);
  CMHAR_CHECK_LAUNCH();
  return 0;
}
