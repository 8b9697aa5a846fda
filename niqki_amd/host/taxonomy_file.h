// taxonomy_file.h -- the file of `niqki --lca`: lines parent<TAB>child over taxon texts.  The parser takes the file's
// bytes (after inflation, where it was gzip'd) and the label texts of the run -- the labels of --collapse, or every
// genome's own name: what parse_label_file (label_file.h) returns as `texts`, so that its `label_of` is genome_taxon --
// and gives every text a taxon id and every taxon its parent, or says which line is wrong.  No engine, no I/O:
// tests/test_taxonomy_file_cpu.py compiles it with a main of its own.
//   * a line ends at '\n' (the last one may lack it); nothing is trimmed, so the '\r' of a CRLF file belongs to the
//     child's text -- the framing rule of the label file; empty lines are skipped
//   * the first TAB of a line splits it: `parent` is the text before it, `child` the rest (further TABs included)
//   * the taxa are the label texts, in their order, followed by every new text in order of first appearance (a line's
//     parent before its child); a taxon is its text
//   * a line whose two texts are equal declares a root and is otherwise ignored; a taxon no line names as a child is a
//     root (its own parent); the same line twice is one line
//   * errors: a line without a TAB, a child under two different parents, a line whose child lies on a cycle
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace nqhost {

struct TaxonomyFile {
  std::vector<std::string> texts;   // per taxon: what the output prints
  std::vector<uint32_t> parent;     // per taxon: its parent, itself for a root
  std::string error;                // empty: the file was taken; else the message, which names `error_line`
  size_t error_line = 0;            // 1-based
};

inline TaxonomyFile parse_taxonomy_file(const char *data, size_t size, const std::vector<std::string> &label_texts) {
  TaxonomyFile out;
  std::unordered_map<std::string, uint32_t> id_of;
  auto taxon_id = [&](const std::string &text) {
    auto it = id_of.find(text);
    if (it != id_of.end()) return it->second;
    const uint32_t id = (uint32_t)out.texts.size();
    out.texts.push_back(text);
    out.parent.push_back(id);
    id_of.emplace(text, id);
    return id;
  };
  for (const std::string &t : label_texts) {   // (label texts are distinct; were two equal, both ids stay and the first is the text's)
    const uint32_t id = (uint32_t)out.texts.size();
    out.texts.push_back(t);
    out.parent.push_back(id);
    id_of.emplace(t, id);
  }
  auto fail = [&](size_t line, const std::string &what) {
    out.error = "line " + std::to_string(line) + ": " + what;
    out.error_line = line;
    out.texts.clear();
    out.parent.clear();
    return out;
  };
  size_t line_no = 0;
  for (size_t at = 0; at < size;) {
    const char *nl = (const char *)std::memchr(data + at, '\n', size - at);
    const size_t end = nl ? (size_t)(nl - data) : size;
    line_no += 1;
    if (end > at) {
      const char *tab = (const char *)std::memchr(data + at, '\t', end - at);
      if (!tab) return fail(line_no, "no TAB (a line is parent<TAB>child)");
      const std::string par(data + at, (size_t)(tab - (data + at))), child(tab + 1, (size_t)(data + end - (tab + 1)));
      const uint32_t p = taxon_id(par), c = taxon_id(child);
      if (p != c) {
        if (out.parent[c] != c && out.parent[c] != p)
          return fail(line_no, "child '" + child + "' is under two parents, '" + out.texts[out.parent[c]] + "' and '" + par + "'");
        // the new edge closes a cycle iff the child is the parent's ancestor already (what is there has no cycle, so
        // the walk ends at a root within as many steps as there are taxa)
        uint32_t a = p;
        for (size_t steps = 0; steps < out.parent.size() && a != c && out.parent[a] != a; ++steps) a = out.parent[a];
        if (a == c) return fail(line_no, "child '" + child + "' lies on a cycle: it is an ancestor of its parent '" + par + "'");
        out.parent[c] = p;
      }
    }
    at = end + 1;
  }
  return out;
}

}  // namespace nqhost
