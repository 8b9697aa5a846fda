// linkage_text.h -- the three texts of the linkage phase (--mst, --linkage, --tree) as plain functions over the arrays
// niqki_linkage returns and the genomes' names.  No engine and no I/O: a writer appends to a string and hands it to
// `sink` (anything callable with a const std::string &) whenever it has grown to kLinkageTextChunk, and once at the
// end, so tests/test_linkage_text_cpu.py drives them from a stand-alone program.  Nothing here recurses: a hierarchy
// may be one chain of all genomes.
//
//   mst       nameLo<TAB>nameHi<TAB>jaccard, the forest edges in edge order; jaccard = count / F, %g
//   linkage   name<TAB>name of merge_into<TAB>jaccard, one line per genome in index order; a root: name<TAB>name<TAB>0
//   tree      Newick, one tree per root, roots in index order, one per line, each ending ';'.  A merge at `count` has
//             height 1 - count / F, leaves are at 0, a branch length is the parent's height minus the node's own, %g.
//             For genome p the genomes g with merge_into[g] == p are grouped by equal merge_count, descending; each
//             group makes ONE internal node whose children are the node built so far for p (first; initially the leaf
//             p) and the complete subtrees of the group's g in ascending id: ties are multifurcations, which is exactly
//             the single-linkage dendrogram.  Leaf labels: the name in single quotes, inner quotes doubled.  A
//             singleton is 'name';
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

namespace nqhost {

constexpr size_t kLinkageTextChunk = size_t(4) << 20;

inline void linkage_number(std::string &text, double v) {
  char num[64];
  const int n = snprintf(num, sizeof num, "%g", v);
  text.append(num, (size_t)n);
}

template <class Sink>
void write_mst(const std::vector<uint32_t> &edge_lo, const std::vector<uint32_t> &edge_hi, const std::vector<uint32_t> &edge_count,
               const std::vector<std::string> &names, uint32_t F, Sink &&sink) {
  std::string text;
  for (size_t e = 0; e < edge_lo.size(); ++e) {
    text += names[edge_lo[e]];
    text += '\t';
    text += names[edge_hi[e]];
    text += '\t';
    linkage_number(text, (double)edge_count[e] / F);
    text += '\n';
    if (text.size() >= kLinkageTextChunk) { sink(text); text.clear(); }
  }
  sink(text);
}

template <class Sink>
void write_linkage(const std::vector<uint32_t> &merge_into, const std::vector<uint32_t> &merge_count,
                   const std::vector<std::string> &names, uint32_t F, Sink &&sink) {
  std::string text;
  for (size_t g = 0; g < merge_into.size(); ++g) {
    text += names[g];
    text += '\t';
    text += names[merge_into[g]];
    text += '\t';
    linkage_number(text, (double)merge_count[g] / F);
    text += '\n';
    if (text.size() >= kLinkageTextChunk) { sink(text); text.clear(); }
  }
  sink(text);
}

template <class Sink>
void write_tree(const std::vector<uint32_t> &merge_into, const std::vector<uint32_t> &merge_count,
                const std::vector<std::string> &names, uint32_t F, Sink &&sink) {
  const uint32_t N = (uint32_t)merge_into.size();
  // the children of every genome: descending count, then ascending id
  std::vector<uint32_t> start(N + 1, 0), ch(N);
  for (uint32_t g = 0; g < N; ++g) if (merge_into[g] != g) start[merge_into[g] + 1] += 1;
  for (uint32_t g = 0; g < N; ++g) start[g + 1] += start[g];
  {
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t g = 0; g < N; ++g) if (merge_into[g] != g) ch[at[merge_into[g]]++] = g;   // (ascending id)
  }
  for (uint32_t p = 0; p < N; ++p)
    std::stable_sort(ch.begin() + start[p], ch.begin() + start[p + 1], [&](uint32_t a, uint32_t b) { return merge_count[a] > merge_count[b]; });
  const auto height = [&](uint32_t count) { return 1.0 - (double)count / F; };
  // the height of a genome's complete subtree: its last group's, a leaf's 0
  const auto top = [&](uint32_t g) { return start[g] == start[g + 1] ? 0.0 : height(merge_count[ch[start[g + 1] - 1]]); };
  std::string text;
  const auto open = [&](uint32_t g) {   // one '(' per group, the leaf, its branch up to the first group
    const uint32_t b = start[g], e = start[g + 1];
    for (uint32_t i = b; i < e; ++i) if (i == b || merge_count[ch[i]] != merge_count[ch[i - 1]]) text += '(';
    text += '\'';
    for (const char c : names[g]) {
      if (c == '\'') text += '\'';
      text += c;
    }
    text += '\'';
    if (b < e) {
      text += ':';
      linkage_number(text, height(merge_count[ch[b]]) - 0.0);
    }
  };
  struct Frame { uint32_t p, i; };
  std::vector<Frame> stack;
  for (uint32_t root = 0; root < N; ++root) {
    if (merge_into[root] != root) continue;
    open(root);
    stack.push_back({root, 0});
    while (!stack.empty()) {
      Frame &f = stack.back();
      const uint32_t b = start[f.p], e = start[f.p + 1];
      if (f.i > 0) {   // the subtree of child i - 1 is written: its branch
        const uint32_t g = ch[b + f.i - 1];
        text += ':';
        linkage_number(text, height(merge_count[g]) - top(g));
      }
      if (b + f.i == e) {
        if (b < e) text += ')';
        stack.pop_back();
        continue;
      }
      const uint32_t g = ch[b + f.i];
      if (f.i > 0 && merge_count[g] != merge_count[ch[b + f.i - 1]]) {   // the next group: the node so far becomes its first child
        text += "):";
        linkage_number(text, height(merge_count[g]) - height(merge_count[ch[b + f.i - 1]]));
      }
      text += ',';
      f.i += 1;
      open(g);
      stack.push_back({g, 0});   // (f is dead from here)
    }
    text += ";\n";
    if (text.size() >= kLinkageTextChunk) { sink(text); text.clear(); }
  }
  sink(text);
}

}  // namespace nqhost
