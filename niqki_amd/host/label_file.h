// label_file.h -- the file of `niqki --collapse`: lines label<TAB>member, what --cluster and --derep write.  The parser
// takes the file's bytes (after inflation, where it was gzip'd) and the names of the indexed genomes and gives every
// genome a label id and every id its text, or says which line is wrong.  No engine, no I/O: tests/test_label_file_cpu.py
// compiles it with a main of its own.
//   * a line ends at '\n' (the last one may lack it); nothing is trimmed, so the '\r' of a CRLF file belongs to the
//     member's name -- the framing rule of the program's other inputs; empty lines are skipped
//   * the first TAB of a line splits it: `label` is any text, `member` (the rest, further TABs included) a genome name
//     exactly as indexed; the line applies to every genome that carries that name
//   * a label is its text: the same text on two lines is one label
//   * a genome that no line names is a label of its own, named by its own name
//   * errors: a line without a TAB, a member no genome carries, a member under two different labels
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace nqhost {

struct LabelFile {
  std::vector<uint32_t> label_of;   // per genome: its label, an index into `texts`
  std::vector<std::string> texts;   // per label: what the output prints
  std::string error;                // empty: the file was taken; else the message, which names `error_line`
  size_t error_line = 0;            // 1-based
};

inline LabelFile parse_label_file(const char *data, size_t size, const std::vector<std::string> &names) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  LabelFile out;
  out.label_of.assign(names.size(), kNone);
  std::unordered_map<std::string, std::vector<uint32_t>> carriers;
  for (size_t g = 0; g < names.size(); ++g) carriers[names[g]].push_back((uint32_t)g);
  std::unordered_map<std::string, uint32_t> id_of;
  auto label_id = [&](const std::string &text) {
    auto it = id_of.find(text);
    if (it != id_of.end()) return it->second;
    const uint32_t id = (uint32_t)out.texts.size();
    out.texts.push_back(text);
    id_of.emplace(text, id);
    return id;
  };
  auto fail = [&](size_t line, const std::string &what) {
    out.error = "line " + std::to_string(line) + ": " + what;
    out.error_line = line;
    out.label_of.clear();
    out.texts.clear();
    return out;
  };
  size_t line_no = 0;
  for (size_t at = 0; at < size;) {
    const char *nl = (const char *)std::memchr(data + at, '\n', size - at);
    const size_t end = nl ? (size_t)(nl - data) : size;
    line_no += 1;
    if (end > at) {
      const char *tab = (const char *)std::memchr(data + at, '\t', end - at);
      if (!tab) return fail(line_no, "no TAB (a line is label<TAB>member)");
      const std::string label(data + at, (size_t)(tab - (data + at))), member(tab + 1, (size_t)(data + end - (tab + 1)));
      const auto who = carriers.find(member);
      if (who == carriers.end()) return fail(line_no, "no indexed genome is named '" + member + "'");
      const uint32_t id = label_id(label);
      for (uint32_t g : who->second) {
        if (out.label_of[g] != kNone && out.label_of[g] != id)
          return fail(line_no, "member '" + member + "' is under two labels, '" + out.texts[out.label_of[g]] + "' and '" + label + "'");
        out.label_of[g] = id;
      }
    }
    at = end + 1;
  }
  for (size_t g = 0; g < names.size(); ++g)
    if (out.label_of[g] == kNone) out.label_of[g] = label_id(names[g]);
  return out;
}

}  // namespace nqhost
