// report_file.h -- the file of `niqki --report`: the taxon tally of a run (niqki_tally_read) as text, one line per
// taxon in the manner of a read classifier's report.  The formatter takes the taxon texts and parents of the run
// (taxonomy_file.h), the four arrays and the totals of the tally and F, the number of sketch slots, and gives the text
// of the file.  No engine, no I/O: tests/test_report_file_cpu.py compiles it with a main of its own.
//   * a line is <pct>\t<clade>\t<direct>\t<depth>\t<mean>\t<indent><text>\n
//   * the first two lines are always there, with zeros too: `unclassified` (the queries without a hit), then
//     `no_common_taxon` (the queries whose considered hits lie in two trees); clade = direct = the count, '-' in the
//     depth and mean columns, no indent
//   * then every taxon with clade > 0 in pre-order; the roots, and the children of a taxon, by clade descending, then
//     by taxon id ascending (the ids are taxonomy_file.h's: the label texts first, then first appearance)
//   * pct is %.2f of 100 * clade / queries (0.00 when there are no queries); mean is %g of clade_best / (clade * F), the
//     mean jaccard of the best hits of the clade's queries, as -O prints a jaccard; indent is two blanks per depth
//   * a text is printed as it is, TABs included: it is the last column
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace nqhost {

struct ReportTotals {
  uint64_t queries = 0, classified = 0, no_hit = 0, no_common = 0;
};

inline std::string report_text(const std::vector<std::string> &texts, const std::vector<uint32_t> &parent, const std::vector<uint64_t> &direct,
                               const std::vector<uint64_t> &clade, const std::vector<uint64_t> &direct_best,
                               const std::vector<uint64_t> &clade_best, const ReportTotals &totals, uint32_t F) {
  (void)direct_best;   // (not printed: a leaf's clade_best is its direct_best)
  const size_t n = std::min({texts.size(), parent.size(), direct.size(), clade.size(), clade_best.size()});
  std::string out;
  char buf[128];
  const auto head = [&](uint64_t c) {   // <pct>\t<clade>\t
    const double pct = totals.queries ? 100.0 * (double)c / (double)totals.queries : 0.0;
    out.append(buf, (size_t)snprintf(buf, sizeof buf, "%.2f\t%llu\t", pct, (unsigned long long)c));
  };
  const struct { const char *name; uint64_t count; } outside[2] = {{"unclassified", totals.no_hit}, {"no_common_taxon", totals.no_common}};
  for (const auto &o : outside) {
    head(o.count);
    out.append(buf, (size_t)snprintf(buf, sizeof buf, "%llu\t-\t-\t", (unsigned long long)o.count));
    out += o.name;
    out += '\n';
  }
  // the taxa with a clade, as lists of children in the order they are written
  std::vector<uint32_t> order;
  for (size_t t = 0; t < n; ++t)
    if (clade[t] && parent[t] < n) order.push_back((uint32_t)t);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return clade[a] != clade[b] ? clade[a] > clade[b] : a < b; });
  std::vector<uint32_t> first(n + 2, 0);   // children of taxon t: kids[first[t] .. first[t + 1]); the roots under the index n
  const auto home = [&](uint32_t t) { return parent[t] == t ? n : (size_t)parent[t]; };
  for (uint32_t t : order) first[home(t) + 1] += 1;
  for (size_t t = 0; t <= n; ++t) first[t + 1] += first[t];
  std::vector<uint32_t> kids(order.size()), at(first.begin(), first.end() - 1);
  for (uint32_t t : order) kids[at[home(t)]++] = t;
  // pre-order without recursion (a taxonomy may be thousands of levels deep): a stack of (taxon, depth)
  std::vector<std::pair<uint32_t, uint32_t>> stack;
  for (uint32_t j = first[n + 1]; j-- > first[n];) stack.emplace_back(kids[j], 0u);
  size_t written = 0;
  while (!stack.empty() && written < order.size()) {   // (every taxon once: a cycle in `parent` cannot be reached from a root)
    const uint32_t t = stack.back().first, d = stack.back().second;
    stack.pop_back();
    written += 1;
    head(clade[t]);
    const double mean = (double)clade_best[t] / ((double)clade[t] * (double)F);
    out.append(buf, (size_t)snprintf(buf, sizeof buf, "%llu\t%u\t%g\t", (unsigned long long)direct[t], d, mean));
    out.append((size_t)d * 2, ' ');
    out += texts[t];
    out += '\n';
    for (uint32_t j = first[t + 1]; j-- > first[t];) stack.emplace_back(kids[j], d + 1);
  }
  return out;
}

}  // namespace nqhost
