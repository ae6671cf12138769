// Batch assembly from a device-resident corpus (gfx950): one launch gathers
// the rows of a batch out of a flat token store into right-padded [B, L]
// token tensors, for one or two sides (source and target) at once.
//
// A side's store is the tokens of all its rows back to back (int32) and an
// int64 [n_rows + 1] offset array (a corpus may hold more than 2^31 tokens;
// row ids are int32). Row b of a side's output is the first min(len, L)
// tokens of store row idx[b], then PAD (0) up to L -- bitwise what the host's
// pad_rows builds.
//
// The kernel trusts nothing it reads from device memory: an id outside
// [0, n_rows), or offsets that are negative, decreasing or past the end of
// the token buffer, give an all-PAD row; a row longer than L is cut at L.
// Each such (row, side) bumps the optional `bad` counter word, which the
// host reads at log points (ops/kernels/batch.py check_gather_rows): a wrong
// batch plan is an error message, never an out-of-bounds access.
//
// The launch moves on the order of 100 KB and is launch-bound, so it is kept
// plain: one 64-lane wave per output row, lanes along the row (coalesced
// dword loads -- row starts in the flat store have no alignment beyond the
// token's own 4 bytes -- and coalesced 4- or 8-byte stores), four rows per
// workgroup, sides over blockIdx.y.
#include "tdg_api.h"
#include "tdg_common.h"

namespace tdg {

struct GatherSide {
  const int* tokens;         // flat store
  const long long* offsets;  // [n_rows + 1]
  long long n_tokens;        // words in `tokens`
  void* out;                 // [B, L] int64 or int32
  int n_rows;
  int L;
};

struct GatherArgs {
  GatherSide side[2];
  const int* idx;  // [B] store row ids
  unsigned* bad;   // counter word, or null
  int B;
  int out64;
};

constexpr int GATHER_WAVE = 64;
constexpr int GATHER_ROWS = 4;  // rows (waves) per workgroup

__global__ __launch_bounds__(GATHER_WAVE* GATHER_ROWS) void gather_rows_kernel(const GatherArgs a) {
  const GatherSide& s = a.side[blockIdx.y];
  const int lane = threadIdx.x % GATHER_WAVE;
  const int b = blockIdx.x * GATHER_ROWS + threadIdx.x / GATHER_WAVE;
  if (b >= a.B) return;
  const int id = a.idx[b];
  long long start = 0, len = 0;
  bool bad = true;
  if (id >= 0 && id < s.n_rows) {
    start = s.offsets[id];
    len = s.offsets[id + 1] - start;
    bad = start < 0 || len < 0 || start > s.n_tokens || len > s.n_tokens - start;
    if (bad) start = len = 0;
  }
  if (len > s.L) {
    len = s.L;
    bad = true;
  }
  if (bad && a.bad && lane == 0) atomicAdd(a.bad, 1u);
  const int* __restrict__ row = s.tokens + start;
  const size_t o = (size_t)b * (size_t)s.L;
  const int n = (int)len;
  if (a.out64) {
    long long* __restrict__ out = static_cast<long long*>(s.out) + o;
    for (int c = lane; c < s.L; c += GATHER_WAVE) out[c] = c < n ? (long long)row[c] : 0ll;
  } else {
    int* __restrict__ out = static_cast<int*>(s.out) + o;
    for (int c = lane; c < s.L; c += GATHER_WAVE) out[c] = c < n ? row[c] : 0;
  }
}

}  // namespace tdg

using namespace tdg;

// out0 [B, L0] (and with nsides == 2 out1 [B, L1]) = rows idx[0, B) of the
// side's store, right-padded with PAD; out64: int64 outputs (else int32);
// ntok*: words in the token buffer; bad: device counter word or null. No
// allocation, no synchronisation: capturable. -1: nsides outside [1, 2];
// -2: B < 1; -3: a side's L < 1; -4: a side's n_rows < 0 (nothing launched).
extern "C" int tdg_gather_rows(int nsides, const int* idx, int B, int out64, const int* tok0,
                               const long long* off0, int nrows0, long long ntok0, void* out0,
                               int L0, const int* tok1, const long long* off1, int nrows1,
                               long long ntok1, void* out1, int L1, unsigned* bad,
                               hipStream_t st) {
  if (nsides < 1 || nsides > 2) return -1;
  if (B < 1) return -2;
  if (L0 < 1 || (nsides == 2 && L1 < 1)) return -3;
  if (nrows0 < 0 || (nsides == 2 && nrows1 < 0)) return -4;
  GatherArgs a;
  a.side[0] = GatherSide{tok0, off0, ntok0, out0, nrows0, L0};
  a.side[1] = nsides == 2 ? GatherSide{tok1, off1, ntok1, out1, nrows1, L1} : a.side[0];
  a.idx = idx;
  a.bad = bad;
  a.B = B;
  a.out64 = out64;
  const dim3 grid((B + GATHER_ROWS - 1) / GATHER_ROWS, nsides);
  hipLaunchKernelGGL(gather_rows_kernel, grid, dim3(GATHER_WAVE * GATHER_ROWS), 0, st, a);
  return 0;
}
