// nq_registers.hip -- niqki_registers / niqki_sketch_registers' device passes: per genome (or query sketch) the histogram
// of the HyperLogLog register in the top H bits of its cells.
//
// hist is u32 [n][B], B = 2^H + 1: hist[j][c >> M] counts row j's valid cells (c < 2^W) with that register value,
// hist[j][2^H] its cells that are not valid; every row sums to the number of cells read.  Both kernels ADD into hist, so
// the caller presets it to zero, and both give one workgroup = one wavefront a rectangle of cells:
//   store pass   64 consecutive columns of the store (u16 [f_local][cap], 0xFFFF empty) x one chunk of rows: a row of
//                them is one 128-byte line, and every lane owns one genome
//   row pass     one sketch (int32 [F]) x one chunk of its cells, 64 consecutive cells (256 bytes) a step: every lane
//                owns a sixty-fourth of the sketch
// Either way a lane keeps B counters of its own in LDS, laid out [bin][lane]: the address of a lane's counter is
// bin * 64 + lane, so the 64 lanes of a step hit 64 different words on 32 banks twice over -- no conflict within a lane
// group -- and no two lanes ever share a counter.  The update is the LDS's own add (no value comes back, so a wavefront
// does not wait for a round trip per cell); it is not there to settle a race.  Counters are 32-bit: 2^16 cells of one
// genome may fall into one bin (S = 16).
// The rows are cut into chunks so that a small index still fills the device (nq_registers launch shape below), and a
// chunk's counters leave with global atomic adds: the store pass one per (genome, bin), where the 64 x B words of a
// wavefront's genomes are contiguous in hist and go out 256 bytes an instruction; the row pass one per bin after a
// sum over its lanes.  Integer adds commute, so hist is the same bit for bit whatever the chunking.  No barrier beyond
// the wavefront's own, no spin, and every loop runs a count fixed at launch.  DESIGN.md 4.6j.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr uint32_t kRegUnroll = 8;        // loads in flight per lane
constexpr uint32_t kRegWaves = 4096;      // wavefronts a launch aims at: 16 per CU
constexpr uint32_t kRegMinRows = 64;      // store pass: rows below which a chunk is not cut further
constexpr uint32_t kRegMinCells = 4096;   // row pass: cells below which a chunk is not cut further

// bin of a cell as the store holds it (v < 2^W or 0xFFFF) and as a sketch row does (any int32)
__device__ __forceinline__ uint32_t reg_bin(uint32_t v, uint32_t R, uint32_t M, uint32_t n_reg) { return v < R ? v >> M : n_reg; }

}  // namespace

// grid (column groups, row chunks), 64 threads; dynamic LDS: B x 64 words
__global__ __launch_bounds__(64) void store_registers_kernel(const uint16_t *store, uint64_t cap, uint32_t f_local, uint32_t begin, uint32_t end,
                                                            uint32_t R, uint32_t M, uint32_t n_reg, uint32_t chunk_rows, uint32_t *hist) {
  extern __shared__ uint32_t cnt[];   // [B][64]
  const uint32_t lane = threadIdx.x, B = n_reg + 1u;
  const uint64_t c0 = (uint64_t)(begin / 64u + blockIdx.x) * 64u;   // the group's first column: a line of every row starts here
  const uint64_t c = c0 + lane;
  const bool mine = c >= begin && c < end;
  const uint32_t r0 = blockIdx.y * chunk_rows;
  const uint32_t r1 = f_local - r0 < chunk_rows ? f_local : r0 + chunk_rows;
  for (uint32_t b = 0; b < B; ++b) cnt[b * 64u + lane] = 0;
  if (mine) {
    const uint16_t *col = store + c;
    uint32_t r = r0;
    for (; r + kRegUnroll <= r1; r += kRegUnroll) {
      uint32_t v[kRegUnroll];
#pragma unroll
      for (uint32_t k = 0; k < kRegUnroll; ++k) v[k] = col[(uint64_t)(r + k) * cap];
#pragma unroll
      for (uint32_t k = 0; k < kRegUnroll; ++k) atomicAdd(&cnt[reg_bin(v[k], R, M, n_reg) * 64u + lane], 1u);
    }
    for (; r < r1; ++r) atomicAdd(&cnt[reg_bin(col[(uint64_t)r * cap], R, M, n_reg) * 64u + lane], 1u);
  }
  __syncthreads();   // (one wavefront: orders the lanes' counters before the others read them)
  // the group's 64 x B words of hist are contiguous: word o belongs to column c0 + o / B, bin o % B
  const uint64_t first = c0 > begin ? (c0 - begin) * B : 0;            // hist word of the group's first live column
  const uint32_t skip = c0 < begin ? (uint32_t)(begin - c0) * B : 0;   // group words before it (the range starts inside the group)
  const uint64_t live = (end - c0 < 64u ? end - c0 : 64u) * (uint64_t)B;
  for (uint32_t o = skip + lane; o < live; o += 64u) {
    const uint32_t x = cnt[(o % B) * 64u + o / B];
    if (x) atomicAdd(hist + first + (o - skip), x);
  }
}

// grid (sketches, cell chunks), 64 threads; dynamic LDS: B x 64 words
__global__ __launch_bounds__(64) void row_registers_kernel(const int32_t *sk, uint32_t F, uint32_t R, uint32_t M, uint32_t n_reg, uint32_t chunk_cells,
                                                          uint32_t *hist) {
  extern __shared__ uint32_t cnt[];   // [B][64]
  const uint32_t lane = threadIdx.x, B = n_reg + 1u;
  const int32_t *row = sk + (uint64_t)blockIdx.x * F;
  const uint32_t i0 = blockIdx.y * chunk_cells;
  const uint32_t i1 = F - i0 < chunk_cells ? F : i0 + chunk_cells;
  for (uint32_t b = 0; b < B; ++b) cnt[b * 64u + lane] = 0;
  uint32_t i = i0 + lane;
  for (; i + (kRegUnroll - 1u) * 64u < i1; i += kRegUnroll * 64u) {
    uint32_t v[kRegUnroll];
#pragma unroll
    for (uint32_t k = 0; k < kRegUnroll; ++k) v[k] = (uint32_t)row[i + k * 64u];   // (a negative cell is a large unsigned one)
#pragma unroll
    for (uint32_t k = 0; k < kRegUnroll; ++k) atomicAdd(&cnt[reg_bin(v[k], R, M, n_reg) * 64u + lane], 1u);
  }
  for (; i < i1; i += 64u) atomicAdd(&cnt[reg_bin((uint32_t)row[i], R, M, n_reg) * 64u + lane], 1u);
  __syncthreads();
  // lane l sums bins l and l + 64 over the lanes, each lane starting at another column of its bin's row (other banks)
  for (uint32_t b = lane; b < B; b += 64u) {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 64u; ++j) sum += cnt[b * 64u + ((j + lane) & 63u)];
    if (sum) atomicAdd(hist + (uint64_t)blockIdx.x * B + b, sum);
  }
}

// Launch shape: enough chunks for kRegWaves wavefronts, no chunk below the minimum, chunk lengths a multiple of what an
// unrolled step takes (the last chunk takes what is left).
static uint32_t chunk_len(uint32_t total, uint64_t groups, uint32_t min_len, uint32_t step) {
  uint64_t chunks = (kRegWaves + groups - 1) / groups;
  const uint64_t most = total / min_len ? total / min_len : 1;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  uint64_t len = (total + chunks - 1) / chunks;
  len = (len + step - 1) / step * step;
  return (uint32_t)(len < total ? len : total);
}

hipError_t launch_store_registers(const Derived &d, const uint16_t *store, uint64_t cap, uint32_t f_local, uint32_t begin, uint32_t end,
                                  uint32_t *hist, hipStream_t stream) {
  if (begin >= end || f_local == 0) return hipSuccess;
  const uint32_t n_reg = 1u << d.H, B = n_reg + 1u;
  const uint32_t groups = (end - 1u) / 64u - begin / 64u + 1u;
  const uint32_t len = chunk_len(f_local, groups, kRegMinRows, kRegUnroll);
  hipLaunchKernelGGL(store_registers_kernel, dim3(groups, (f_local + len - 1) / len), dim3(64), (size_t)B * 64 * 4, stream, store, cap, f_local,
                     begin, end, d.R, d.M, n_reg, len, hist);
  return hipGetLastError();
}

hipError_t launch_row_registers(const Derived &d, const int32_t *sketches, uint32_t n, uint32_t *hist, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t n_reg = 1u << d.H, B = n_reg + 1u;
  const uint32_t len = chunk_len(d.F, n, kRegMinCells, kRegUnroll * 64u);
  hipLaunchKernelGGL(row_registers_kernel, dim3(n, (d.F + len - 1) / len), dim3(64), (size_t)B * 64 * 4, stream, sketches, d.F, d.R, d.M, n_reg,
                     len, hist);
  return hipGetLastError();
}

}  // namespace nq
