// reseg.hip — the matching step of the Resegmentation pipeline (PA/pipelines/resegmentation.py:217-243): for every window, how
// many frames each speaker of the given diarization and each local speaker of the model disagree on.  The reference calls
// permutate(..., cost_func=mae_cost_func) once per window (PA/utils/permutation.py:83-157): a Python loop that builds an
// [n, n] cost matrix of torch.mean(|Y - y|) over {0,1} columns.  On {0,1} data |Y - y| summed over frames is a Hamming
// distance, so the whole loop is one launch here:
//   count[c, i, j] = #{ l < Lt : refpad[row[c] + l, i] != segpad[c, l0 + l, j] }          n = max(K, S) <= 32
// refpad / segpad are the two operands widened to n columns with zeros (resegmentation.py:217-228); reference rows at or
// beyond Tr read as zero.  The assignment itself (scipy.optimize.linear_sum_assignment) stays on the host: the caller divides
// by Lt in float32 as torch.mean does.
//
// One workgroup (4 wavefronts of 64) per window, stateless, no global atomics.  Frames are taken MATCH_TILE_WORDS x 64 at a
// time: a wavefront packs 64 frames of one column into one 64-bit word with a ballot (lane l holds frame w * 64 + l; lanes past
// Lt, padded columns and rows outside [0, Tr) vote 0, so both operands are zero there and add nothing), the 2 n columns of the
// tile go to LDS, and each thread then keeps up to MATCH_PAIRS (i, j) pairs: popcount(ref[i] ^ seg[j]) word by word.  Only u8
// loads from the two inputs and plain int32 vector stores to the output.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(reseg)        // check ids 0x88x: 0x880 decision read, 0x881 reference read, 0x882 LDS word, 0x883 count write

namespace {

constexpr int MATCH_MAX_N = 32;            // widest padded side (the K <= 32 bound of dzn_cluster_activations)
constexpr int MATCH_TILE_WORDS = 16;       // 16 x 64 = 1024 frames per LDS tile: 2 x 32 x 16 x 8 B = 8 KiB
constexpr int MATCH_THREADS = 256;
constexpr int MATCH_PAIRS = MATCH_MAX_N * MATCH_MAX_N / MATCH_THREADS;      // 4 pairs per thread at n = 32

__global__ __launch_bounds__(MATCH_THREADS) void match_counts_kernel(const uint8_t* __restrict__ seg,
                                                                     const uint8_t* __restrict__ ref, int C, int L, int S,
                                                                     int Tr, int K, const int32_t* __restrict__ row, int l0,
                                                                     int Lt, int n, int32_t* __restrict__ count) {
  __shared__ unsigned long long bits[2][MATCH_MAX_N][MATCH_TILE_WORDS];      // [0]: reference columns, [1]: local speakers
  const int c = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = row[c];
  const uint8_t* segc = seg + (int64_t)c * L * S;
  const int words = (Lt + 63) >> 6;
  int acc[MATCH_PAIRS];
#pragma unroll
  for (int q = 0; q < MATCH_PAIRS; ++q) acc[q] = 0;

  for (int w0 = 0; w0 < words; w0 += MATCH_TILE_WORDS) {
    const int tw = min(MATCH_TILE_WORDS, words - w0);
    // pack: word-rows are dealt to the wavefronts, every lane of a wavefront takes every trip of both loops (ballot)
    for (int w = wave; w < tw; w += MATCH_THREADS / 64) {
      const int l = ((w0 + w) << 6) + lane;              // frame of the trimmed window
      const bool in_window = l < Lt;
      const int64_t rr = r0 + l;                         // reference row
      const bool in_ref = in_window && rr >= 0 && rr < Tr;
      for (int k = 0; k < n; ++k) {
        int vr = 0, vs = 0;
        if (in_ref && k < K) {
          DZN_CHECK(rr * K + k < (int64_t)Tr * K, 0x881, rr);
          vr = ref[rr * K + k] != 0;
        }
        if (in_window && k < S) {
          DZN_CHECK((int64_t)(l0 + l) * S + k < (int64_t)L * S, 0x880, l0 + l);
          vs = segc[(int64_t)(l0 + l) * S + k] != 0;
        }
        const unsigned long long br = __ballot(vr), bs = __ballot(vs);
        if (lane == 0) {
          DZN_CHECK(k < MATCH_MAX_N && w < MATCH_TILE_WORDS, 0x882, k * MATCH_TILE_WORDS + w);
          bits[0][k][w] = br;
          bits[1][k][w] = bs;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MATCH_PAIRS; ++q) {
      const int p = threadIdx.x + q * MATCH_THREADS;
      if (p < n * n) {
        const int i = p / n, j = p - i * n;
        int d = 0;
        for (int w = 0; w < tw; ++w) d += __popcll(bits[0][i][w] ^ bits[1][j][w]);
        acc[q] += d;
      }
    }
    __syncthreads();                                     // the next tile overwrites the words
  }
  int32_t* out = count + (int64_t)c * n * n;
#pragma unroll
  for (int q = 0; q < MATCH_PAIRS; ++q) {
    const int p = threadIdx.x + q * MATCH_THREADS;
    if (p < n * n) {
      DZN_CHECK((int64_t)c * n * n + p < (int64_t)C * n * n, 0x883, p);
      out[p] = acc[q];
    }
  }
}

}  // namespace

extern "C" int dzn_match_counts(const uint8_t* d_seg, const uint8_t* d_ref, int32_t C, int32_t L, int32_t S, int32_t Tr,
                                int32_t K, const int32_t* d_row, int32_t l0, int32_t Lt, int32_t* d_count, void* stream) {
  if (C < 0 || L < 1 || S < 1 || K < 0 || Tr < 0 || l0 < 0 || Lt < 1 || (int64_t)l0 + Lt > L) return DZN_E_INVALID;
  const int n = K > S ? K : S;
  if (n > MATCH_MAX_N) return DZN_E_INVALID;
  if (C == 0) return DZN_OK;
  if (!d_seg || !d_row || !d_count || (!d_ref && K > 0 && Tr > 0)) return DZN_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(match_counts_kernel, dim3((unsigned)C), dim3(MATCH_THREADS), 0, st, d_seg, d_ref, C, L, S, Tr, K, d_row,
                     l0, Lt, n, d_count);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
