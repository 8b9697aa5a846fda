// size_estimate_main.cpp -- niqki_amd/host/size_estimate.h as a stand-alone program, for tests/test_registers_ref_cpu.py
// (and the place for a sanitizer build of the header: g++ -fsanitize=address,undefined on this one file).
// Standard input, a request per line:
//   E <S> <H> <2^H + 1 counts>                       ->  <kmers %.0f>\t<status>
//   C <S> <H> <count> <2^H + 1 counts of the query> <2^H + 1 counts of the genome>
//                                                    ->  <jaccard %g>:<cq %g>:<cg %g>, or <jaccard %g>:-:-
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../niqki_amd/host/size_estimate.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char what = 0;
    uint32_t S = 0, H = 0, count = 0;
    in >> what >> S >> H;
    if (!in || H > 6 || S > 16 || (what != 'E' && what != 'C')) return 1;
    if (what == 'C') in >> count;
    const size_t B = (size_t(1) << H) + 1;
    std::vector<uint32_t> hist(what == 'C' ? 2 * B : B);
    for (auto &x : hist) in >> x;
    if (!in) return 1;
    if (what == 'E') {
      const nqsize::Estimate e = nqsize::estimate(hist.data(), S, H);
      std::printf("%.0f\t%s\n", e.kmers, nqsize::status_text(e.status));
    } else {
      const nqsize::Containment c = nqsize::containment(count, S, nqsize::estimate(hist.data(), S, H), nqsize::estimate(hist.data() + B, S, H));
      if (c.defined) std::printf("%g:%g:%g\n", c.jaccard, c.cq, c.cg);
      else std::printf("%g:-:-\n", c.jaccard);
    }
  }
  return 0;
}
