// ubench_sketch.hip -- the sketch kernel alone, without Python: N random ACGT genomes of L bases in HBM,
// launch_sketch timed with HIP events; the filtered result is compared with the unfiltered (exact) pass.
// Includes the product source directly, so -D switches of nq_sketch.hip can be tried per binary:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude tools/ubench_sketch.hip -o tools/bin/ubench_sketch
//   tools/bin/ubench_sketch [n_genomes=1024] [len=5000000] [reps=3] [S=15]
#define NQ_SKETCH_CLOCK 1
#include "../niqki_amd/csrc/nq_sketch.hip"
#include "../niqki_amd/csrc/nq_sketch_reads.hip"   // (launch_sketch reaches the other units' kernels)
#include "../niqki_amd/csrc/nq_densify.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

__global__ void fill_acgt(uint8_t *p, uint64_t n, uint64_t seed) {
  uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 32;
  if (i >= n) return;
  uint64_t z = (i / 32 + seed) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  for (int j = 0; j < 32 && i + j < n; ++j) p[i + j] = (uint8_t)((0x54474341u >> (8 * ((z >> (2 * j)) & 3))) & 0xFFu);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
  const uint32_t n = argc > 1 ? atoi(argv[1]) : 1024;
  const uint64_t L = argc > 2 ? atoll(argv[2]) : 5000000;
  const int reps = argc > 3 ? atoi(argv[3]) : 3;
  const uint32_t S = argc > 4 ? atoi(argv[4]) : 15;
  nq::Derived d{};
  d.K = 31; d.S = S; d.W = 12; d.H = 4; d.M = 8; d.F = 1u << S; d.R = 1u << 12; d.mask_m = 255; d.max_rem = 15;
  d.min_score = 0; d.slot_begin = 0; d.slot_end = d.F; d.kmer_mask = (1ULL << 62) - 1;
  uint8_t *seq; uint64_t *ro; int32_t *sk, *sk2;
  CK(hipMalloc(&seq, n * L + 4096));
  CK(hipMalloc(&ro, (n + 1) * 8));
  CK(hipMalloc(&sk, (size_t)n * d.F * 4));
  CK(hipMalloc(&sk2, (size_t)n * d.F * 4));
  hipLaunchKernelGGL(fill_acgt, dim3((uint32_t)((n * L / 32 + 255) / 256 + 1)), dim3(256), 0, 0, seq, n * L + 4096, 12345ull);
  std::vector<uint64_t> h(n + 1);
  for (uint32_t i = 0; i <= n; ++i) h[i] = i * L;
  CK(hipMemcpy(ro, h.data(), (n + 1) * 8, hipMemcpyHostToDevice));
  nq::SketchArgs a{};
  a.d = d; a.seqs = seq; a.rec_off = ro; a.entry_rec = nullptr; a.sketches = sk; a.splits = 1;
  a.accumulate = 0; a.densify = 1;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const nq::SketchPlan plan = nq::sketch_plan(d, L, 1, true, false, true, nq::sketch_switches());
  CK(nq::launch_sketch(a, n, plan, 0));
  CK(hipDeviceSynchronize());
  {   // (no tick of an earlier launch may pass for one of the last launch's: a workgroup that records none reads as zeros)
    const std::vector<unsigned long long> zero(18 * nq::kWaveTraceWgs, 0ull);
    CK(hipMemcpyToSymbol(HIP_SYMBOL(nq::nq_sketch_wave), zero.data(), zero.size() * 8));
  }
  CK(hipEventRecord(e0));
  for (int r = 0; r < reps; ++r) CK(nq::launch_sketch(a, n, plan, 0));
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  const double kmers = (double)reps * n * (L - 31);
  printf("sketch: %u x %llu bp, %.3f ms per launch, %.1f G k-mers/s\n", n, (unsigned long long)L, ms / reps, kmers / (ms * 1e-3) / 1e9);
  {
    unsigned long long clk[2];
    CK(hipMemcpyFromSymbol(clk, HIP_SYMBOL(nq::nq_sketch_clk), 16));
    printf("workgroup 0: %llu shader cycles in %.1f us = %.3f GHz\n", clk[0], clk[1] * 0.01, clk[0] / (clk[1] * 10.0));
  }
  {
    // When the waves of a SIMD finish (line form only: records of 2^21 bases and more).  Wave w runs on SIMD w % 4; the
    // times are shares of the loop, from the tick before it to the one behind the barrier after it, means over the
    // recorded workgroups of the last launch.  The bound prices the time a SIMD spends with two waves and with one at
    // the rates measured with two and one wave per SIMD (1.21 x and 1.90 x the cycles of four, profiles/r03); three
    // waves count as free.
    std::vector<unsigned long long> wv(18 * nq::kWaveTraceWgs);
    CK(hipMemcpyFromSymbol(wv.data(), HIP_SYMBOL(nq::nq_sketch_wave), wv.size() * 8));
    double share[4][4] = {}, all[4] = {}, idle = 0, loop_us = 0, two = 0, one = 0;
    uint32_t wgs = 0;
    for (uint32_t b = 0; b < nq::kWaveTraceWgs && b < n; ++b) {
      const unsigned long long *t = &wv[18 * b];
      if (t[1] <= t[0]) continue;   // (not the line form: nothing recorded)
      const double dur = (double)(t[1] - t[0]);
      for (int s = 0; s < 4; ++s) {
        double f[4];
        for (int j = 0; j < 4; ++j) f[j] = (double)(t[2 + 4 * j + s] - t[0]) / dur;
        std::sort(f, f + 4);
        for (int j = 0; j < 4; ++j) { share[s][j] += f[j]; all[j] += f[j] / 4; }
        two += (f[2] - f[1]) / 4; one += (f[3] - f[2]) / 4; idle += (1.0 - f[3]) / 4;
      }
      loop_us += dur * 0.01;
      ++wgs;
    }
    if (wgs) {
      printf("wave finish times, shares of the loop (%u workgroups, loop %.1f us on average)\n", wgs, loop_us / wgs);
      printf("%-6s %8s %8s %8s %8s\n", "SIMD", "first", "second", "third", "last");
      for (int s = 0; s < 4; ++s) printf("%-6d %8.4f %8.4f %8.4f %8.4f\n", s, share[s][0] / wgs, share[s][1] / wgs, share[s][2] / wgs, share[s][3] / wgs);
      printf("%-6s %8.4f %8.4f %8.4f %8.4f\n", "all", all[0] / wgs, all[1] / wgs, all[2] / wgs, all[3] / wgs);
      printf("share of the loop a SIMD runs two waves %.4f, one wave %.4f, none (until the barrier) %.4f\n", two / wgs, one / wgs, idle / wgs);
      printf("bound of the gain from level waves: %.4f of the loop (two waves x (1 - 1/1.21) + one wave x (1 - 1/1.90))\n",
             two / wgs * (1.0 - 1.0 / 1.21) + one / wgs * (1.0 - 1.0 / 1.90));
    }
  }
  if (getenv("SK_TRACE")) {
    std::vector<unsigned long long> tr(3 * 8192);
    CK(hipMemcpyFromSymbol(tr.data(), HIP_SYMBOL(nq::nq_sketch_trace), tr.size() * 8));
    unsigned long long t0 = ~0ull, t1 = 0;
    const uint32_t nb = n < 8192 ? n : 8192;
    for (uint32_t b = 0; b < nb; ++b) { if (tr[3 * b] < t0) t0 = tr[3 * b]; if (tr[3 * b + 1] > t1) t1 = tr[3 * b + 1]; }
    printf("last launch: first start to last end %.1f us\n", (t1 - t0) * 0.01);
    FILE *f = fopen(getenv("SK_TRACE"), "w");
    for (uint32_t b = 0; b < nb; ++b) {
      const unsigned long long id = tr[3 * b + 2];
      const uint32_t hw = (uint32_t)id, xcc = (uint32_t)(id >> 32) & 15u;
      // HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13
      fprintf(f, "%u %.2f %.2f xcc %u se %u sh %u cu %u\n", b, (tr[3 * b] - t0) * 0.01, (tr[3 * b + 1] - t0) * 0.01, xcc,
              (hw >> 13) & 7u, (hw >> 12) & 1u, (hw >> 8) & 15u);
    }
    fclose(f);
  }
  // exactness: the unfiltered pass on the first genomes
  const uint32_t nc = n < 8 ? n : 8;
  setenv("NIQKI_SKETCH_FILTER", "0", 1);
  a.sketches = sk2;
  CK(nq::launch_sketch(a, nc, nq::sketch_plan(d, L, 1, true, false, true, nq::sketch_switches()), 0));
  CK(hipDeviceSynchronize());
  std::vector<int32_t> x((size_t)nc * d.F), y((size_t)nc * d.F);
  CK(hipMemcpy(x.data(), sk, x.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(y.data(), sk2, y.size() * 4, hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (size_t i = 0; i < x.size(); ++i) bad += x[i] != y[i];
  printf("filtered vs exact pass on %u genomes: %zu cells differ\n", nc, bad);
  return bad != 0;
}
