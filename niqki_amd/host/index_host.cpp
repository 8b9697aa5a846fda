// index_host.cpp -- file-level drivers of the `niqki` host program.  Moves the
// bytes of the input files into page-locked memory and calls the gfx950 engine
// through the C ABI (include/niqki_hip.h): record framing (the reference's
// Biogetline), sketching, counting and sorting all happen on the GPU.
#include "index_host.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <future>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../csrc/nq_pack.h"
#include "file_reader.h"
#include "label_file.h"
#include "taxonomy_file.h"
#include "report_file.h"
#include "linkage_text.h"
#include "piece_reader.h"
#include "seqio.h"

namespace nqhost {

namespace {
bool exists_test(const std::string &name) {  // src/niqki_index.h:150-153
  struct stat st;
  return stat(name.c_str(), &st) == 0;
}
// default ostream << double: 6 significant digits, %g style (src/niqki_index.cpp:550,:758)
std::string fmt_double(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}
constexpr size_t kBatchBytes = size_t(1) << 30;   // dump import: bytes per GPU call

constexpr size_t kWholeBatchFiles = 64;                // files per GPU call (whole-file mode)
constexpr size_t kWholeBatchBytes = size_t(3) << 29;   // ... or 1.5 GB
constexpr size_t kReaderBufs = 2 * kWholeBatchFiles + 32;
// Gzip files inflated on the device: a file is one wavefront's serial job there and the device runs up to 2048 of them
// at once (eight per CU with the window's last 8 KB in LDS; 1024 with all of it), so a batch takes as long as its
// longest file whatever it holds -- batches of up to 2048 files (their bytes are a third of the plain ones'), 4 GB
// of file bytes or 12 GB of inflated ones.
constexpr size_t kGzBatchFiles = 2048;
constexpr size_t kGzBatchWireBytes = size_t(4) << 30;
constexpr size_t kGzBatchRawBytes = size_t(12) << 30;
constexpr size_t kGzReaderBufs = 2 * kGzBatchFiles + 64;
}  // namespace

// Files of one GPU call (whole-file mode): one sketch per file.
struct Index::Batch {
  std::vector<OrderedFileReader::File *> files;
  std::vector<std::string> names;
  size_t bytes = 0;       // bytes that cross PCIe
  size_t raw_bytes = 0;   // bytes the device holds once packed / gzip'd files are their own bytes again (gzip: as announced)
  size_t n_gz = 0;
};

void Index::check_on(niqki_index *h, int rc, const char *what) {
  if (rc == NIQKI_OK) return;
  throw std::runtime_error(std::string(what) + ": " + niqki_status_string(rc) + " (" + niqki_last_error(h) + ")");
}

void Index::check_group(int rc, const char *what) const {
  if (rc == NIQKI_OK) return;
  throw std::runtime_error(std::string(what) + ": " + niqki_status_string(rc) + " (" + niqki_group_last_error(grp_) + ")");
}

// ---- the calls an engine may lack ---------------------------------------------------
namespace {
// per Index::Feature, in its order: the symbols it needs and the text of an engine without one of them
const struct {
  const char *symbols[3];
  const char *text;
} kFeatures[] = {
    {{"niqki_append_begin", "niqki_append_slots", "niqki_append_cancel"}, "this engine cannot merge dumps"},
    {{"niqki_dereplicate_from"}, "this engine has no dereplication"},
    {{"niqki_retain"}, "this engine cannot drop genomes"},
    {{"niqki_unite"}, "this engine cannot unite genomes"},
    {{"niqki_neighbors_range", "niqki_cluster"}, "this engine has no self-join"},
    {{"niqki_dereplicate"}, "this engine has no dereplication"},
    {{"niqki_linkage"}, "this engine has no linkage"},
    {{"niqki_set_labels", "niqki_audit"}, "this engine has no label audit"},
    {{"niqki_set_taxonomy", "niqki_staged_query_lca"}, "this engine has no LCA query"},
    {{"niqki_staged_cover"}, "this engine has no cover"},
    {{"niqki_registers", "niqki_staged_registers"}, "this engine cannot read sketch registers"},
    {{"niqki_set_sizes", "niqki_staged_query_contained"}, "this engine cannot select hits by containment"},
    {{"niqki_set_labels", "niqki_staged_query_collapsed"}, "this engine has no collapsed query"},
    {{"niqki_tally_begin", "niqki_tally_read"}, "this engine has no taxon tally"},
};
template <typename Fn>
Fn engine_call(const char *name) { return (Fn)dlsym(RTLD_DEFAULT, name); }
}  // namespace

const char *Index::lacks(Feature f) {
  for (const char *symbol : kFeatures[(size_t)f].symbols)
    if (symbol && !engine_call<void *>(symbol)) return kFeatures[(size_t)f].text;
  return nullptr;
}

template <typename Fn>
Fn Index::need(Feature f, const char *name) const {
  if (lacks(f) || grp_) throw std::runtime_error(kFeatures[(size_t)f].text);
  return engine_call<Fn>(name);
}
// the call as the header declares it: NEED(COVER, niqki_staged_cover)(h_, ...)
#define NEED(feature, call) need<decltype(&call)>(Feature::feature, #call)

void Index::refuse(const std::string &text) {
  outfile->close();
  (void)::unlink(out_path_.c_str());
  throw std::runtime_error(text);
}

// One capacity retry for every call that fills hit lists: `sets` x n lists (off, hc, hg of a Hits), room for `first`
// hits in each to begin with.  call(cap) runs the engine call; while it answers that cap is too small and cap is below
// `limit` (the most the lists can hold: then the answer is an error), cap becomes twice the larger of itself and the
// largest total the engine reported in off[n], but no more than limit, and the call runs again.  Returns the last answer.
template <typename Set, typename Call>
static int fill_lists(Set *sets, size_t n_sets, size_t n, uint64_t first, uint64_t limit, Call &&call) {
  for (size_t s = 0; s < n_sets; ++s) sets[s].off.resize(n + 1);
  for (uint64_t cap = first;;) {
    for (size_t s = 0; s < n_sets; ++s) {
      sets[s].hc.resize(cap);
      sets[s].hg.resize(cap);
    }
    const int rc = call(cap);
    if (rc != NIQKI_E_CAPACITY || cap >= limit) return rc;
    for (size_t s = 0; s < n_sets; ++s) cap = std::max(cap, sets[s].off[n]);
    cap = std::min(limit, cap * 2);
  }
}

// One handle per GPU: with n_gpus > 1 shard r owns the slots of rank r (niqki_group_slot_range) on device
// device + r.  dump_header != nullptr: the handles are made for a streamed dump import.
void Index::make_shards(const niqki_params &p0, int device, int n_gpus, const uint8_t *dump_header) {
  if (n_gpus < 1 || n_gpus > 64) throw std::runtime_error("--gpus must be in 1..64");
  for (int r = 0; r < n_gpus; ++r) {
    niqki_params p = p0;
    p.device = n_gpus > 1 ? (device < 0 ? 0 : device) + r : device;
    // test hook: all shards on one device (a 1-GPU box emulating N; the library then moves the
    // exchanged data with device-to-device copies instead of RCCL)
    if (n_gpus > 1 && std::getenv("NIQKI_SHARDS_ON_ONE_DEVICE")) p.device = device;
    if (n_gpus > 1) niqki_group_slot_range((uint32_t)r, (uint32_t)n_gpus, dump_header ? ((const uint32_t *)dump_header)[0] : p.S, &p.slot_begin, &p.slot_end);
    niqki_index *h = nullptr;
    check_on(nullptr, dump_header ? niqki_import_begin(&p, dump_header, &h) : niqki_create(&p, &h),
             dump_header ? "niqki_import_begin" : "niqki_create");
    sh_.push_back(h);
  }
  h_ = sh_[0];
}

Index::Index(uint32_t ilF, uint32_t iK, uint32_t iW, uint32_t iH, const std::string &out_filename,
             double min_fract, int device, int n_gpus, int resident_mib, uint32_t itop_k) {
  niqki_params p{};
  p.K = iK; p.S = ilF; p.W = iW; p.H = iH;
  p.resident_mib = resident_mib > 0 ? (uint32_t)resident_mib : 0u;
  p.top_k = top_k = itop_k;
  p.min_score = niqki_min_score(min_fract, ilF);
  make_shards(p, device, n_gpus, nullptr);
  K = iK; W = iW; H = iH; lF = ilF; F = 1u << ilF; min_score = p.min_score;
  open_group_and_output(out_filename);
}

namespace {
// The streamed walk over a dump file, shared by the loading constructor (-L) and merge_dump (--merge): header, then the
// buckets in groups of whole slots (the payload of a 100k-genome index is 13.6 GB), then the names.  A dump this
// program wrote is a file of size-tagged gzip members (gzio.h): they are inflated side by side by the reader threads, a
// window ahead; any other gzip file (the reference's dumps are one member) comes through zlib's stream.  Either way the
// bytes arrive in pieces, and the walk over the buckets' size words -- the one serial thing about the format -- runs
// over memory, not over a reader call per bucket.
// header: the 24 header bytes, once, before any slot (it refuses a dump by throwing); slots: the payload of whole
// slots [s0, s1), in order; names: the header's N lines behind the buckets (src/niqki_index.cpp:91-95) are appended.
void walk_dump(const std::string &dump_file, const std::function<void(const uint8_t *)> &header,
               const std::function<void(uint32_t, uint32_t, const uint8_t *, size_t)> &slots, std::vector<std::string> &names) {
  std::unique_ptr<TaggedGzReader> tagged;
  std::unique_ptr<GzReader> plain;
  if (TaggedGzReader::probe(dump_file)) {
    // (a file that starts like one of ours but does not go on that way -- another gzip file appended, a member re-written
    // by some tool -- is still a gzip file: zlib's stream reads it, as the reference's zstr would)
    try { tagged.reset(new TaggedGzReader(dump_file, host_threads())); } catch (const std::exception &) { tagged.reset(); }
  }
  if (!tagged) plain.reset(new GzReader(dump_file));
  std::vector<uint8_t> buf, piece;
  size_t p = 0;   // parse position in buf
  auto more = [&]() -> bool {   // appends the stream's next piece
    if (tagged) {
      if (!tagged->next(piece)) return false;
    } else {
      piece.resize(size_t(4) << 20);
      piece.resize(plain->read(piece.data(), piece.size()));
      if (piece.empty()) return false;
    }
    buf.insert(buf.end(), piece.begin(), piece.end());
    return true;
  };
  auto need = [&](size_t n) -> bool {
    while (buf.size() - p < n)
      if (!more()) return false;
    return true;
  };
  if (!need(24)) throw std::runtime_error("'" + dump_file + "' is not a niqki dump");
  uint32_t hdr[6];
  std::memcpy(hdr, buf.data(), 24);
  p = 24;
  header(buf.data());
  const uint32_t F = 1u << hdr[0], R = 1u << hdr[3];
  uint32_t s0 = 0;
  size_t g0 = p;   // where the slots not yet handed over start in buf
  auto flush = [&](uint32_t s1) {
    slots(s0, s1, buf.data() + g0, p - g0);
    buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)p);   // (what is left is less than one piece)
    p = g0 = 0;
    s0 = s1;
  };
  for (uint32_t s = 0; s < F; ++s) {
    for (uint32_t fp = 0; fp < R; ++fp) {
      if (!need(4)) throw std::runtime_error("'" + dump_file + "' is truncated");
      uint32_t size;
      std::memcpy(&size, buf.data() + p, 4);
      if (!need(4 + (size_t)size * 4)) throw std::runtime_error("'" + dump_file + "' is truncated");
      p += 4 + (size_t)size * 4;
    }
    if (p - g0 >= kBatchBytes / 8) flush(s + 1);
  }
  flush(F);
  while (more()) {}
  for (uint32_t i = 0; i < hdr[5]; ++i) {
    const uint8_t *b0 = buf.data() + p, *e0 = buf.data() + buf.size();
    const uint8_t *nl = p < buf.size() ? (const uint8_t *)memchr(b0, '\n', (size_t)(e0 - b0)) : nullptr;
    const uint8_t *end = nl ? nl : e0;
    names.emplace_back(p < buf.size() ? std::string((const char *)b0, (size_t)(end - b0)) : std::string());
    p = nl ? (size_t)(nl + 1 - buf.data()) : buf.size();
  }
}
}  // namespace

Index::Index(const std::string &dump_file, bool pretty, const std::string &out_filename, int device, int n_gpus,
             int resident_mib, uint32_t itop_k) {
  pretty_printing = pretty;
  walk_dump(
      dump_file,
      [&](const uint8_t *hdr) {
        niqki_params prm{};
        prm.resident_mib = resident_mib > 0 ? (uint32_t)resident_mib : 0u;
        prm.top_k = top_k = itop_k;   // (the dump does not hold it: niqki_import_begin takes it from the params)
        make_shards(prm, device, n_gpus, hdr);   // every shard keeps its own slots of the stream
        niqki_params q{};
        niqki_get_params(h_, &q);
        K = q.K; W = q.W; H = q.H; lF = q.S; F = 1u << q.S; min_score = q.min_score;
      },
      [&](uint32_t s0, uint32_t s1, const uint8_t *data, size_t len) {
        uint64_t used = 0;
        for (auto *h : sh_) check(niqki_import_slots(h, s0, s1, data, len, &used), "niqki_import_slots");
      },
      filenames);
  open_group_and_output(out_filename);
}

void Index::open_group_and_output(const std::string &out_filename) {
  if (sh_.size() > 1)
    check(niqki_group_create(sh_.data(), (uint32_t)sh_.size(), 0, (uint32_t)sh_.size(), nullptr, &grp_), "niqki_group_create");
  out_path_ = out_filename;
  outfile.reset(new ParallelTextWriter(out_filename, host_threads()));
}

Index::~Index() {
  // (after an error pending text may fail to be written once more: the error that ended the run has been reported)
  try {
    if (outfile) outfile->close();
  } catch (...) {
  }
  if (grp_) niqki_group_destroy(grp_);
  for (auto *h : sh_) niqki_destroy(h);
}

// src/niqki_index.cpp:126-138, including its message
void Index::select_best_H(double genome_size) {
  uint32_t chosen = H;
  for (auto *h : sh_) check(niqki_select_best_H(h, genome_size, &chosen), "select_best_H");
  H = chosen;
  std::cout << "I chosed H=" << H << std::endl;
}

void Index::compute_sketch(const std::string &reference, std::vector<int32_t> &sketch) const {
  sketch.assign(F, -1);
  uint64_t off[2] = {0, reference.size()};
  check(niqki_sketch(h_, (const uint8_t *)reference.data(), off, 1, nullptr, 1, sketch.data(), NIQKI_MEM_HOST), "niqki_sketch");
}

void Index::insert_sketch(const std::vector<int32_t> &sketch, uint32_t genome_id) {
  if (genome_id != niqki_genome_count(h_)) throw std::runtime_error("insert_sketch: ids must be consecutive");
  for (auto *h : sh_) check(niqki_insert(h, sketch.data(), 1, NIQKI_MEM_HOST), "niqki_insert");  // each shard keeps its slots
}

query_output Index::query_sketch(const std::vector<int32_t> &sketch) const {
  const uint32_t n = niqki_genome_count(h_);
  std::vector<uint32_t> hc(n ? n : 1), hg(n ? n : 1);
  uint64_t off[2] = {0, 0};
  if (grp_) {  // the shards' partial hit vectors summed on the host (a single sketch: API parity, not a fast path)
    const uint64_t stride = NIQKI_ROW_STRIDE(n);
    std::vector<uint16_t> sum(std::max<uint64_t>(stride, 2), 0), part(std::max<uint64_t>(stride, 2));
    for (auto *h : sh_) {
      check(niqki_query_counts(h, sketch.data(), 1, part.data(), stride, NIQKI_MEM_HOST), "niqki_query_counts");
      for (uint32_t i = 0; i < n; ++i) sum[i] = (uint16_t)(sum[i] + part[i]);
    }
    check(niqki_hits_from_counts(h_, sum.data(), 1, stride, 0, n, off, hc.data(), hg.data(), n, NIQKI_MEM_HOST), "niqki_hits_from_counts");
  } else
  check(niqki_query(h_, sketch.data(), 1, off, hc.data(), hg.data(), n, NIQKI_MEM_HOST), "niqki_query");
  query_output r;
  for (uint64_t i = 0; i < off[1]; ++i) r.push_back({hc[i], hg[i]});
  return r;
}

// ---- insertion / query drivers ---------------------------------------------------

Index::Share Index::rank_share(size_t n) const {
  Share s;
  s.per = (uint32_t)((n + sh_.size() - 1) / sh_.size());
  for (size_t r = 0, lo = 0; r < sh_.size(); ++r, lo += s.per) s.n_entry.push_back((uint32_t)std::min<size_t>(s.per, n - std::min(n, lo)));
  return s;
}

// stage the files of a batch: one entry per file (insert_file_whole / query_file_whole,
// src/niqki_index.cpp:442-456, :505-519); multi-GPU: rank_share's files to each shard

// prefetch: only start the batch's host-to-device copy (niqki_stage_raw_prefetch); the stage_batch call
// that follows for the same batch takes those bytes
void Index::stage_batch(Batch &b, bool prefetch) {
  auto stage = [&](niqki_index *h, size_t lo, size_t hi) {
    for (;;) {
      std::vector<const uint8_t *> ptr(hi - lo);
      std::vector<uint64_t> off(hi - lo + 1, 0);
      std::vector<uint8_t> type(hi - lo), status(hi - lo, 0);
      for (size_t i = lo; i < hi; ++i) {
        ptr[i - lo] = b.files[i]->buf.p;
        off[i - lo + 1] = off[i - lo] + b.files[i]->buf.size;
        type[i - lo] = b.files[i]->packed ? (uint8_t)'a'
                       : b.files[i]->gz   ? (uint8_t)(data_type(b.names[i]) | NIQKI_FILE_GZIP)
                                          : (uint8_t)data_type(b.names[i]);
      }
      niqki_raw_batch rb{};
      rb.file_ptr = ptr.data();
      rb.file_off = off.data();
      rb.file_type = type.data();
      rb.n_files = (uint32_t)(hi - lo);
      rb.file_status = status.data();
      niqki_stage_info info{};
      const int rc = prefetch ? niqki_stage_raw_prefetch(h, &rb) : niqki_stage_raw(h, &rb, NIQKI_MEM_HOST, &info, nullptr);
      if (rc == NIQKI_E_GZIP) {
        // files the device would not inflate (damaged, several members, ...): through zlib here -- which decides what
        // they yield, or throws, exactly as for a run without the device inflate -- and the batch again (every pass
        // leaves fewer gzip files, so this ends)
        size_t redone = 0;
        for (size_t i = lo; i < hi; ++i)
          if (status[i - lo] && b.files[i]->gz) {
            read_file_bytes(b.names[i], b.files[i]->buf);
            b.files[i]->gz = false;
            ++redone;
          }
        if (redone) continue;
      }
      check_on(h, rc, "niqki_stage_raw");
      return;
    }
  };
  const Share s = rank_share(b.files.size());
  for (size_t r = 0, lo = 0; r < sh_.size(); lo += s.n_entry[r++])
    if (s.n_entry[r]) stage(sh_[r], lo, lo + s.n_entry[r]);
}

namespace {
struct Lap {  // adds the time since construction (or the last lap) to an accumulator
  using clk = std::chrono::steady_clock;
  clk::time_point t = clk::now();
  void to(double &acc) {
    const auto n = clk::now();
    acc += std::chrono::duration<double>(n - t).count();
    t = n;
  }
};
}  // namespace

void Index::staged_insert(const Share &s) {
  if (grp_) check_group(niqki_group_staged_insert(grp_, s.per, s.n_entry.data()), "niqki_group_staged_insert");
  else check(niqki_staged_insert(h_), "niqki_staged_insert");
}

void Index::staged_hits(const Share &s, Hits &h) {
  h.collapsed = h.lca = false;
  h.qsize.clear();
  if (grp_) group_query_staged(s, h);
  else query_staged(s.n_entry[0], h);
}

// the staged batch of b's files: sketched and inserted
void Index::flush_insert(Batch &b) {
  Lap lap;
  staged_insert(rank_share(b.files.size()));
  for (auto &nm : b.names) filenames.push_back(nm);
  lap.to(t_dev_);
}

// the first capacity of a call that returns the whole lists of n queries: with top_k at most n x k hits (that is
// never too small), else `floor` or `each` per query
static uint64_t first_capacity(uint64_t n, uint64_t top_k, uint64_t longest, uint64_t floor, uint64_t each) {
  return top_k ? std::max<uint64_t>(n * std::min(top_k, longest), 1) : std::max(floor, n * each);
}

// hits of the entries staged on the shards, rank after rank = entry order
void Index::group_query_staged(const Share &s, Hits &h) {
  const size_t G = sh_.size();
  const uint64_t N = niqki_genome_count(h_);
  std::vector<Hits> part(G);   // (off, hc, hg of each rank)
  std::vector<uint64_t *> p_off(G);
  std::vector<uint32_t *> p_hc(G), p_hg(G);
  check_group(fill_lists(part.data(), G, s.per, first_capacity(s.per, top_k, N, uint64_t(1) << 20, 64), (uint64_t)s.per * N,
                         [&](uint64_t cap) {
                           for (size_t r = 0; r < G; ++r) { p_off[r] = part[r].off.data(); p_hc[r] = part[r].hc.data(); p_hg[r] = part[r].hg.data(); }
                           return niqki_group_staged_query(grp_, s.per, s.n_entry.data(), p_off.data(), p_hc.data(), p_hg.data(), cap, NIQKI_MEM_HOST);
                         }),
              "niqki_group_staged_query");
  h.off.assign(1, 0);
  h.hc.clear();
  h.hg.clear();
  for (size_t r = 0; r < G; ++r)
    for (uint32_t i = 0; i < s.n_entry[r]; ++i) {
      h.hc.insert(h.hc.end(), part[r].hc.begin() + part[r].off[i], part[r].hc.begin() + part[r].off[i + 1]);
      h.hg.insert(h.hg.end(), part[r].hg.begin() + part[r].off[i], part[r].hg.begin() + part[r].off[i + 1]);
      h.off.push_back(h.hc.size());
    }
}

void Index::read_labels(const char *option, const std::string &filestr, std::vector<uint32_t> &label_of, std::vector<std::string> &texts) {
  LabelFile lf;
  std::string err;
  try {
    PinnedBuf bytes;
    read_file_bytes(filestr, bytes);
    lf = parse_label_file((const char *)bytes.p, bytes.size, filenames);
    err = lf.error;
  } catch (const std::exception &e) { err = e.what(); }
  if (!err.empty()) refuse(std::string(option) + " '" + filestr + "': " + err);
  label_of = std::move(lf.label_of);
  texts = std::move(lf.texts);
}

void Index::set_collapse(const std::string &filestr) {
  const auto call = NEED(COLLAPSE, niqki_set_labels);
  read_labels("--collapse", filestr, label_of_, label_text_);
  check(call(h_, label_of_.empty() ? nullptr : label_of_.data(), (uint32_t)label_of_.size(), NIQKI_MEM_HOST), "niqki_set_labels");
  collapse_ = true;
}

void Index::set_lca(const std::string &filestr, uint32_t top_permille, const std::string &label_file) {
  const auto call = NEED(LCA, niqki_set_taxonomy);
  LabelFile lf;
  TaxonomyFile tf;
  std::string err, which = "--lca '" + filestr + "'";
  try {
    if (!label_file.empty()) {   // --collapse beside --lca: its labels are the leaves
      PinnedBuf bytes;
      read_file_bytes(label_file, bytes);
      lf = parse_label_file((const char *)bytes.p, bytes.size, filenames);
      if (!lf.error.empty()) which = "--collapse '" + label_file + "'";
    } else {
      lf = parse_label_file(nullptr, 0, filenames);   // every genome its own label under its own name
    }
    err = lf.error;
    if (err.empty()) {
      PinnedBuf bytes;
      read_file_bytes(filestr, bytes);
      tf = parse_taxonomy_file((const char *)bytes.p, bytes.size, lf.texts);
      err = tf.error;
    }
  } catch (const std::exception &e) { err = e.what(); }
  if (!err.empty()) refuse(which + ": " + err);
  taxon_text_ = std::move(tf.texts);
  taxon_parent_ = std::move(tf.parent);
  if (!lf.label_of.empty())
    check(call(h_, lf.label_of.data(), (uint32_t)lf.label_of.size(), taxon_parent_.data(), (uint32_t)taxon_parent_.size(), NIQKI_MEM_HOST), "niqki_set_taxonomy");
  if (!report.empty() && !lf.label_of.empty()) {   // --report: the queries from here on feed the tally
    check(NEED(TALLY, niqki_tally_begin)(h_), "niqki_tally_begin");
    tally_open_ = true;
  }
  lca_permille_ = top_permille;
  lca_ = true;
}

void Index::write_report() {
  const size_t T = taxon_text_.size();
  std::vector<uint64_t> direct(T, 0), clade(T, 0), direct_best(T, 0), clade_best(T, 0);
  ReportTotals totals;
  totals.queries = totals.no_hit = untallied_;
  if (tally_open_) {
    niqki_tally_totals t{};
    check(NEED(TALLY, niqki_tally_read)(h_, direct.data(), clade.data(), direct_best.data(), clade_best.data(), &t, NIQKI_MEM_HOST), "niqki_tally_read");
    totals.queries = t.queries;
    totals.classified = t.classified;
    totals.no_hit = t.no_hit;
    totals.no_common = t.no_common;
  }
  ParallelTextWriter out(report, host_threads());
  out.write(report_text(taxon_text_, taxon_parent_, direct, clade, direct_best, clade_best, totals, F));
  out.close();
}

// hits of the n entries staged on the one GPU
void Index::query_staged(size_t n, Hits &h) {
  const uint64_t N = niqki_genome_count(h_);
  if (lca_) {   // --lca: each entry's taxon in the place of its hits, with the count of its best hit; no entry without a hit
    const auto call = NEED(LCA, niqki_staged_query_lca);
    std::vector<uint32_t> taxon(std::max<size_t>(n, 1)), best(std::max<size_t>(n, 1)), considered(std::max<size_t>(n, 1));
    check(call(h_, lca_permille_, taxon.data(), best.data(), nullptr, considered.data(), NIQKI_MEM_HOST), "niqki_staged_query_lca");
    if (!tally_open_) untallied_ += n;
    h.off.assign(n + 1, 0);
    h.hc.clear();
    h.hg.clear();
    for (size_t i = 0; i < n; ++i) {
      if (considered[i]) {
        h.hc.push_back(best[i]);
        h.hg.push_back(taxon[i]);
      }
      h.off[i + 1] = h.hc.size();
    }
    h.lca = true;
  } else if (collapse_) {   // --collapse: each entry's best hit per label in the place of its hits, at most top_k labels
    const auto call = NEED(COLLAPSE, niqki_staged_query_collapsed);
    const uint64_t L = label_text_.size();
    check(fill_lists(&h, 1, n, first_capacity(n, top_k, L, uint64_t(1) << 16, 8), n * L,
                     [&](uint64_t cap) { return call(h_, h.off.data(), h.hc.data(), h.hg.data(), nullptr, cap, NIQKI_MEM_HOST); }),
          "niqki_staged_query_collapsed");
    h.collapsed = N != 0;
  } else if (cover) {   // --cover: each entry's greedy cover in the place of its hits, at most top_k picks
    const auto call = NEED(COVER, niqki_staged_cover);
    check(fill_lists(&h, 1, n, first_capacity(n, top_k, N, uint64_t(1) << 16, 8), n * N,
                     [&](uint64_t cap) { return call(h_, top_k, h.off.data(), h.hc.data(), h.hg.data(), nullptr, cap, NIQKI_MEM_HOST); }),
          "niqki_staged_cover");
  } else if (min_share) {   // --min-containment: the entries chosen, ordered and cut by their share on the device
    const auto call = NEED(CONTAINED, niqki_staged_query_contained);
    staged_sizes(n, (uint32_t)N, h);
    // (an estimate of 2^40 or more is no size the engine takes: such a hit counts as unsized)
    const auto kmers = [](const nqsize::Estimate &e) { return e.status == nqsize::OK && e.kmers + 0.5 < 1099511627776.0 ? (uint64_t)std::floor(e.kmers + 0.5) : uint64_t(0); };
    if (!sizes_set_) {   // once, at the first query batch: the index is final by then
      std::vector<uint64_t> sizes(N);
      for (uint64_t g = 0; g < N; ++g) sizes[g] = kmers(genome_size_[g]);
      check(NEED(CONTAINED, niqki_set_sizes)(h_, sizes.empty() ? nullptr : sizes.data(), (uint32_t)N, NIQKI_MEM_HOST), "niqki_set_sizes");
      sizes_set_ = true;
    }
    std::vector<uint64_t> qs(std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; ++i) qs[i] = kmers(h.qsize[i]);
    std::vector<uint32_t> shares, unsized(std::max<size_t>(n, 1), 0);
    check(fill_lists(&h, 1, n, first_capacity(n, top_k, N, uint64_t(1) << 16, 8), n * N,
                     [&](uint64_t cap) {
                       shares.resize(cap);
                       return call(h_, qs.data(), contain_mode, min_share, h.off.data(), shares.data(), h.hc.data(), h.hg.data(), unsized.data(), cap,
                                   NIQKI_MEM_HOST);
                     }),
          "niqki_staged_query_contained");
    for (size_t i = 0; i < n; ++i) unsized_hits += unsized[i];
  } else {
    check(fill_lists(&h, 1, n, first_capacity(n, top_k, N, uint64_t(1) << 20, 64), n * N,
                     [&](uint64_t cap) { return niqki_staged_query(h_, h.off.data(), h.hc.data(), h.hg.data(), cap, NIQKI_MEM_HOST); }),
          "niqki_staged_query");
    if (containment) staged_sizes(n, (uint32_t)N, h);   // --containment: the plain list with each entry's two shares
  }
}

void Index::staged_sizes(size_t n, uint32_t N, Hits &h) {
  const auto call = NEED(SIZES, niqki_staged_registers);
  if (!genome_size_ok_) {
    genome_size_ = genome_sizes(N);
    genome_size_ok_ = true;
  }
  const uint32_t B = NIQKI_REGISTER_BINS(H);
  std::vector<uint32_t> hist(std::max<size_t>(n, 1) * B);
  check(call(h_, hist.data(), NIQKI_MEM_HOST), "niqki_staged_registers");
  h.qsize.resize(n);
  for (size_t i = 0; i < n; ++i) h.qsize[i] = nqsize::estimate(hist.data() + i * B, lF, H);
}

std::vector<nqsize::Estimate> Index::genome_sizes(uint32_t n) const {
  const auto call = NEED(SIZES, niqki_registers);
  const uint32_t B = NIQKI_REGISTER_BINS(H);
  std::vector<uint32_t> hist((size_t)std::max<uint32_t>(n, 1) * B);
  check(call(h_, 0, n, hist.data(), NIQKI_MEM_HOST), "niqki_registers");
  std::vector<nqsize::Estimate> sizes(n);
  for (uint32_t g = 0; g < n; ++g) sizes[g] = nqsize::estimate(hist.data() + (size_t)g * B, lF, H);
  return sizes;
}

void Index::sizes_to_file(const std::string &filestr) {
  const std::vector<nqsize::Estimate> sizes = genome_sizes((uint32_t)filenames.size());
  ParallelTextWriter out(filestr, host_threads());
  std::string text;
  char num[64];
  for (size_t g = 0; g < sizes.size(); ++g) {
    text += filenames[g];
    text += '\t';
    text.append(num, (size_t)snprintf(num, sizeof num, "%.0f", sizes[g].kmers));
    text += '\t';
    text += nqsize::status_text(sizes[g].status);
    text += '\n';
    if (text.size() >= (size_t(4) << 20)) { out.write(text); text.clear(); }
  }
  out.write(text);
  out.close();
}

// ... written in entry order
void Index::write_hits(const Hits &h) {
  if (!pretty_printing) {
    query_output one;
    for (size_t i = 0; i < h.names.size(); ++i) {
      one.clear();
      for (uint64_t j = h.off[i]; j < h.off[i + 1]; ++j) one.push_back({h.hc[j], h.hg[j]});
      output_query(one, h.names[i]);
    }
    return;
  }
  // the lines of output_query (:546-553), put together a few megabytes at a time: a batch of lines mode is 65 536
  // entries, and a call per entry -- a vector of hits, a string, a write -- was a third of the writer thread's time
  std::string &text = out_text_;
  text.clear();
  char num[64];
  for (size_t i = 0; i < h.names.size(); ++i) {
    text += h.names[i];
    text += ' ';
    for (uint64_t j = h.off[i]; j < h.off[i + 1]; ++j) {
      if (h.lca) text += h.hg[j] < taxon_text_.size() ? taxon_text_[h.hg[j]] : std::string("no_common_taxon");
      else text += h.collapsed ? label_text_[label_of_[h.hg[j]]] : filenames[h.hg[j]];
      text += ':';
      const int n = snprintf(num, sizeof num, "%g", (double)h.hc[j] / F);
      text.append(num, (size_t)n);
      if (!h.qsize.empty()) {   // --containment: :cq:cg behind the jaccard
        const nqsize::Containment c = nqsize::containment(h.hc[j], lF, h.qsize[i], genome_size_[h.hg[j]]);
        if (c.defined) text.append(num, (size_t)snprintf(num, sizeof num, ":%g:%g", c.cq, c.cg));
        else text += ":-:-";
      }
      text += ' ';
    }
    text += '\n';
    if (text.size() >= (size_t(4) << 20)) { outfile->write(text); text.clear(); }
  }
  outfile->write(text);
}

// The thread that puts the hit lines of a batch together and writes them while the next batch is on the GPU.  It owns
// n_hits Hits that go round: get() waits for a free one (so at most n_hits batches are filled, wait or are written),
// push() hands a filled one over, the thread writes them in push order -- after the first error it only takes them
// back -- and finish() returns when everything pushed is written; `err` holds the first error then.  Lines mode: the
// names are cut out of the piece of input here, and `release` is told when the piece (Hits::keep) is no longer needed.
struct Index::HitsWriter {
  std::string err;
  HitsWriter(Index *ix, size_t n_hits, std::function<void(void *)> release = nullptr)
      : ix_(ix), release_(std::move(release)), pool_(n_hits), th_([this] { run(); }) {
    for (auto &h : pool_) free_.push(&h);
  }
  ~HitsWriter() { finish(); }
  Hits *get() { return free_.pop(); }
  void push(Hits *h) { queue_.push(h); }
  void give_back(Hits *h) {   // (also a Hits that was never pushed: its call failed)
    if (h->keep) release_(h->keep);
    h->keep = nullptr;
    h->name_base = nullptr;
    free_.push_front(h);   // (the next to be taken again: its arrays are warm, the pool's untouched ones cost page faults)
  }
  void finish() {
    queue_.push(nullptr);
    if (th_.joinable()) th_.join();
  }

 private:
  void run() {
    while (Hits *h = queue_.pop()) {
      try {
        if (h->name_base) {   // the header lines of the entries, cut out here instead of on the GPU thread
          h->names.clear();
          h->names.reserve(h->name_at.size());
          for (uint64_t at : h->name_at) h->names.push_back(header_line(h->name_base, h->name_room, at));
        }
        if (err.empty()) ix_->write_hits(*h);
      } catch (const std::exception &e) { err = e.what(); }
      give_back(h);
    }
  }
  Index *ix_;
  std::function<void(void *)> release_;
  std::deque<Hits> pool_;
  Channel<Hits *> free_, queue_;
  std::thread th_;   // (the last member: it runs on the ones above)
};

// ... sketched, queried and handed to the writer thread
void Index::flush_query(Batch &b) {
  Lap lap;
  Hits *h = writer_->get();
  lap.to(t_out_);
  h->names = b.names;
  staged_hits(rank_share(b.files.size()), *h);
  lap.to(t_dev_);
  writer_->push(h);
}

// The files of `paths` in batches: reader threads fill page-locked buffers ahead, the bytes of batch i+1 cross
// to the device (copy stream) while batch i is sketched, inserted or queried and its output written.
void Index::for_each_batch(const std::vector<std::string> &paths, void (Index::*flush)(Batch &)) {
  using clk = std::chrono::steady_clock;
  const bool timing = std::getenv("NIQKI_HOST_TIMING") != nullptr;  // where the wall time goes, on stderr
  double t_wait = 0, t_gpu = 0;
  t_stage_ = t_dev_ = t_out_ = 0;
  const auto t_begin = clk::now();
  // A list of mostly gzip'd files (by their names) is inflated on the device, in the large batches that wants -- if
  // it is long enough: a launch of the device inflate takes one file's time (150 ms for a 5 Mbp genome) however few
  // files it holds, in which a reader thread inflates some 30 files, so below 32 files per reader thread the readers
  // do it (NIQKI_HOST_GPU_INFLATE_MIN sets that number of files; NIQKI_HOST_NO_GPU_INFLATE: always the readers).
  const unsigned n_threads = host_threads();
  size_t n_gz_names = 0, gz_min = size_t(32) * n_threads;
  for (const auto &p : paths) n_gz_names += p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0;
  if (const char *v = std::getenv("NIQKI_HOST_GPU_INFLATE_MIN")) gz_min = (size_t)std::max(0, std::atoi(v));
  const bool gz_list = std::getenv("NIQKI_HOST_NO_GPU_INFLATE") == nullptr && 2 * n_gz_names > paths.size() && n_gz_names >= gz_min;
  OrderedFileReader rd(paths, n_threads, gz_list ? std::min(kGzReaderBufs, 2 * paths.size() + 64) : kReaderBufs,
                       std::getenv("NIQKI_HOST_NO_GPU_INFLATE") ? 0 : gz_list ? 2 : 1);
  size_t i = 0, n_batches = 0;
  auto assemble = [&](Batch &b) {
    const auto t0 = clk::now();
    // the first batches are small (16, 32, 64 files): the GPU and the copy engine start while the reader threads are
    // still page-locking their buffers and filling the pipeline.  (Gzip lists: equal batches of at most 2048 -- a launch
    // of the device inflate takes as long as its longest file however few files it holds, so small batches only cost: on
    // 2048 files 256 + 1024 + 768 gives 3.6 k genomes/s, 1024 + 1024 5.1 k, one batch 5.5 k; on 4096 files
    // 1024 + 2048 + 1024 gives 5.3 k.)
    const size_t gz_batches = (paths.size() + kGzBatchFiles - 1) / kGzBatchFiles;
    const size_t limit = gz_list ? (paths.size() + gz_batches - 1) / std::max<size_t>(gz_batches, 1)
                                 : std::min<size_t>(kWholeBatchFiles, size_t(16) << std::min<size_t>(n_batches++, 8));
    while (b.files.size() < limit && b.bytes < (gz_list ? kGzBatchWireBytes : kWholeBatchBytes) && b.raw_bytes < kGzBatchRawBytes) {
      auto *f = rd.next();
      if (!f) break;
      b.files.push_back(f);
      b.names.push_back(paths[i++]);
      b.bytes += f->buf.size;
      size_t raw = f->buf.size;
      if (f->gz) {   // (the reader checked the trailer: at least 18 bytes, a plausible size)
        const uint8_t *e = f->buf.p + f->buf.size - 4;
        raw = (size_t)e[0] | (size_t)e[1] << 8 | (size_t)e[2] << 16 | (size_t)e[3] << 24;
        if (raw < f->buf.size) raw = 4 * f->buf.size;   // (a file of tagged members: the trailer is its last member's)
        ++b.n_gz;
      }
      b.raw_bytes += raw;
    }
    t_wait += std::chrono::duration<double>(clk::now() - t0).count();
  };
  // The bytes of batch i + 1 cross PCIe while batch i is worked on (the library keeps two prefetch buffers).  Gzip lists
  // (2048 files, gigabytes a batch, readers far ahead of the device): batch i + 1 is put together and sent on its way
  // BEFORE batch i is staged, so the copy runs under batch i's inflate kernel.  Other lists (64 files a batch, readers
  // about as fast as the device): batch i is staged first, so that the readers' buffers are not all spoken for while it
  // runs -- waiting for batch i + 1 up front cost a third of the rate there.
  // Queries: a batch's hit lines are put together and written by a thread of their own while the next batch is on the
  // GPU (HitsWriter: four batches may wait there beside the one being filled and the one being written; output order
  // is batch order).  With thousands of hits per query the text took as long as the GPU calls: 4000 virus-sized genomes
  // against themselves, 0.20 of 0.43 s.
  std::unique_ptr<HitsWriter> writer;
  if (flush == &Index::flush_query) writer.reset(new HitsWriter(this, 6));
  writer_ = writer.get();   // (flush_query runs only from here)
  Batch cur, nxt;
  assemble(cur);
  if (!cur.files.empty()) stage_batch(cur, true);
  while (!cur.files.empty()) {
    if (gz_list) {
      assemble(nxt);
      if (!nxt.files.empty()) stage_batch(nxt, true);
    }
    auto t0 = clk::now();
    Lap lap;
    stage_batch(cur, false);
    lap.to(t_stage_);
    t_gpu += std::chrono::duration<double>(clk::now() - t0).count();
    if (!gz_list) {
      assemble(nxt);
      if (!nxt.files.empty()) stage_batch(nxt, true);
    }
    t0 = clk::now();
    (this->*flush)(cur);
    t_gpu += std::chrono::duration<double>(clk::now() - t0).count();
    for (auto *f : cur.files) rd.release(f);
    cur = std::move(nxt);
    nxt = Batch();
  }
  if (writer) {
    Lap lap;
    writer->finish();
    lap.to(t_out_);
    if (!writer->err.empty()) throw std::runtime_error(writer->err);
  }
  if (timing)
    std::cerr << "[niqki timing] " << paths.size() << " files: total "
              << std::chrono::duration<double>(clk::now() - t_begin).count() << " s, waiting for file bytes " << t_wait
              << " s, GPU calls (copy + frame + sketch + insert/query + output) " << t_gpu << " s (copy + frame "
              << t_stage_ << ", sketch + insert/query " << t_dev_ << ", output " << t_out_ << ")" << std::endl;
}

void Index::insert_file_of_file_whole(const std::string &filestr) {
  std::ifstream in(filestr);
  if (!in) {
    std::cout << "Unable to open the file '" << filestr << "'" << std::endl;
    exit(0);  // src/niqki_index.cpp:464-467
  }
  // the list first (:479-490: lines longer than 2 characters naming an existing
  // file; ids follow the list order), then the files, read in parallel
  std::vector<std::string> paths;
  std::string ref;
  while (!in.eof()) {
    std::getline(in, ref);
    if (ref.size() > 2 && exists_test(ref)) paths.push_back(ref);
    ref.clear();
  }
  for_each_batch(paths, &Index::flush_insert);
}

void Index::query_file_of_file_whole(const std::string &filestr) {
  GzReader in(filestr);
  std::vector<std::string> paths;
  std::string ref;
  while (!in.eof()) {
    in.getline(ref);
    if (exists_test(ref)) paths.push_back(ref);  // :534
    ref.clear();
  }
  for_each_batch(paths, &Index::flush_query);
}

// ---- lines mode: reader thread -> GPU calls (caller's thread) -> writer thread ------

niqki_stage_info Index::stage_lines(niqki_index *h, const uint8_t *raw, size_t size, char type, std::vector<uint64_t> &hdr) {
  const uint64_t off[2] = {0, size};
  const uint8_t type_u8 = (uint8_t)type;
  niqki_raw_batch rb{};
  rb.raw = raw;
  rb.file_off = off;
  rb.file_type = &type_u8;
  rb.n_files = 1;
  rb.lines = 1;
  rb.final = 1;  // pieces hold whole records
  rb.max_entries = (uint32_t)hdr.size();
  niqki_stage_info info{};
  check_on(h, niqki_stage_raw(h, &rb, NIQKI_MEM_HOST, &info, hdr.data()), "niqki_stage_raw");
  return info;
}

size_t Index::deal_lines(const uint8_t *raw, size_t size, char type, std::vector<uint64_t> &hdr, Share &s, std::vector<uint64_t> &name_at) {
  const size_t G = sh_.size();
  std::vector<size_t> cut(G + 1, 0);   // rank r takes raw[cut[r], cut[r + 1])
  cut[G] = size;
  for (size_t r = 1; r < G; ++r) cut[r] = std::max(cut[r - 1], record_cut(raw, size * r / G, type));
  s.per = 0;
  s.n_entry.assign(G, 0);
  name_at.clear();
  for (size_t r = 0; r < G; ++r) {
    if (cut[r + 1] == cut[r]) continue;
    const niqki_stage_info info = stage_lines(sh_[r], raw + cut[r], cut[r + 1] - cut[r], type, hdr);
    s.n_entry[r] = info.n_entry;
    s.per = std::max(s.per, info.n_entry);
    for (uint32_t e = 0; e < info.n_entry; ++e) name_at.push_back(cut[r] + hdr[e]);
    if (info.consumed < cut[r + 1] - cut[r]) return cut[r] + info.consumed;   // more entries than one call takes: the round ends inside this run
  }
  return size;
}

// One entry per record longer than K, named by its header line (insert_file_lines /
// query_file_lines, :383-430).  A reader thread streams the file into page-locked pieces
// that end at a record boundary, this thread runs the GPU calls, a writer thread formats
// and compresses the hits: the three overlap, output order is input order.
void Index::stream_lines(const std::string &filestr, bool insert) {
  using clk = std::chrono::steady_clock;
  const auto t_begin = clk::now();
  uint64_t n_entries_total = 0;
  const char type = data_type(filestr);
  // sketches of one call stay below 2 GB
  const uint32_t max_entries = (uint32_t)std::min<uint64_t>(65536, std::max<uint64_t>(1024, (uint64_t(2) << 30) / ((uint64_t)F * 4)));
  PieceReader reader(filestr, type);
  HitsWriter writer(this, 4, [&reader](void *pc) { reader.release((Piece *)pc); });
  std::string err;
  std::vector<uint64_t> hdr(max_entries), name_at;
  Share share;
  double t_piece = 0, t_frame = 0, t_names = 0, t_engine = 0, t_slot = 0;   // NIQKI_HOST_TIMING: where this thread's time goes
  try {
    for (bool last = false; !last;) {
      Lap lap;
      Piece *pc = reader.next();
      lap.to(t_piece);
      last = pc->last;
      for (size_t at = 0; at < pc->buf.size;) {
        const uint8_t *base = pc->buf.p + at;
        const size_t left = pc->buf.size - at;
        const size_t done = deal_lines(base, left, type, hdr, share, name_at);
        lap.to(t_frame);
        const size_t total = name_at.size();
        n_entries_total += total;
        if (insert && total) {
          for (uint64_t a : name_at) filenames.push_back(header_line(base, left, a));
          lap.to(t_names);
          staged_insert(share);
        } else if (total) {
          Hits *h = writer.get();
          lap.to(t_slot);
          // the writer thread cuts the names out of the piece (it stays alive until then: Piece::refs)
          h->name_base = base;
          h->name_room = left;
          h->name_at.swap(name_at);
          h->keep = pc;
          reader.retain(pc);
          lap.to(t_names);
          try { staged_hits(share, *h); } catch (...) { writer.give_back(h); throw; }
          writer.push(h);
        }
        lap.to(t_engine);
        if (done == 0 && total == 0) break;   // nothing but a header without end
        at += done;
      }
      reader.release(pc);
    }
  } catch (const std::exception &e) {
    err = e.what();
  }
  reader.stop();
  writer.finish();
  if (!err.empty()) throw std::runtime_error(err);
  if (!writer.err.empty()) throw std::runtime_error(writer.err);
  if (std::getenv("NIQKI_HOST_TIMING"))
    std::cerr << "[niqki timing] lines mode: " << n_entries_total << " entries in "
              << std::chrono::duration<double>(clk::now() - t_begin).count() << " s (this thread: waiting for file bytes " << t_piece
              << ", copy + frame " << t_frame << ", names " << t_names << ", sketch + insert/query " << t_engine
              << ", waiting for the writer " << t_slot << ")" << std::endl;
}

void Index::insert_file_lines(const std::string &filestr) { stream_lines(filestr, true); }

void Index::query_file_lines(const std::string &filestr) { stream_lines(filestr, false); }

void Index::output_query(const query_output &toprint, const std::string &queryname) {
  if (pretty_printing) {  // :546-553
    std::string line = queryname + " ";
    for (const auto &h : toprint) {
      line += filenames[h.second];
      line += ':';
      line += fmt_double((double)h.first / F);
      line += ' ';
    }
    line += '\n';
    outfile->write(line);
  } else {  // :555-564 (unreachable from the reference CLI, kept for API parity)
    outfile->write(queryname + "\n");
    uint32_t size = (uint32_t)toprint.size();
    outfile->write(&size, 4);
    for (const auto &h : toprint) {
      outfile->write(&h.second, 4);
      outfile->write(&h.first, 4);
    }
  }
}

// ---- matrix ----------------------------------------------------------------------

void Index::output_matrix_row(const uint16_t *counts, const std::string &queryname) {
  // query_range threshold (:600-606) + output_matrix (:747-763)
  std::string line = queryname + "\t";
  const size_t n = filenames.size();
  for (size_t j = 0; j < n; ++j) {
    double v = counts[j] >= min_score ? (double)counts[j] / F : 0.0;
    line += fmt_double(v);
    line += '\t';
  }
  line += '\n';
  outfile->write(line);
}

void Index::query_matrix() {
  std::string head = "##Names\t";  // :615-619
  for (const auto &nm : filenames) { head += nm; head += '\t'; }
  head += '\n';
  outfile->write(head);
  const uint32_t n = (uint32_t)filenames.size();
  const uint64_t stride = NIQKI_ROW_STRIDE(n);
  const uint32_t rows = 256;
  std::vector<uint16_t> counts((size_t)rows * std::max<uint64_t>(stride, 2));
  std::vector<uint16_t> part(grp_ ? counts.size() : 0);
  for (uint32_t t0 = 0; t0 < n; t0 += rows) {
    const uint32_t t1 = std::min(n, t0 + rows);
    check(niqki_matrix_range(h_, t0, t1, counts.data(), stride, NIQKI_MEM_HOST), "niqki_matrix_range");
    for (size_t r = 1; r < sh_.size(); ++r) {   // slot shards: co-occurrence counts add up over the slots
      check(niqki_matrix_range(sh_[r], t0, t1, part.data(), stride, NIQKI_MEM_HOST), "niqki_matrix_range");
      const size_t m = (size_t)(t1 - t0) * stride;
      for (size_t i = 0; i < m; ++i) counts[i] = (uint16_t)(counts[i] + part[i]);
    }
    for (uint32_t t = t0; t < t1; ++t) output_matrix_row(counts.data() + (size_t)(t - t0) * stride, filenames[t]);
  }
}

// ---- self-join --------------------------------------------------------------------

void Index::query_neighbors() {
  const auto call = NEED(SELF_JOIN, niqki_neighbors_range);
  const uint32_t N = (uint32_t)filenames.size(), rows = 1024;
  Hits h;
  for (uint32_t t0 = 0; t0 < N; t0 += rows) {
    const uint32_t t1 = std::min(N, t0 + rows), n = t1 - t0;
    h.names.assign(filenames.begin() + t0, filenames.begin() + t1);
    // (capacity as query_staged)
    check(fill_lists(&h, 1, n, first_capacity(n, top_k, N, uint64_t(1) << 20, 64), (uint64_t)n * N,
                     [&](uint64_t cap) { return call(h_, t0, t1, h.off.data(), h.hc.data(), h.hg.data(), cap, NIQKI_MEM_HOST); }),
          "niqki_neighbors_range");
    write_hits(h);
  }
}

// lines label<TAB>member: the groups in the index order of their label (a member of its own group), inside a group the
// label's own line first, then the other members in index order
void Index::write_groups(const std::string &filestr, const std::vector<uint32_t> &labels, uint32_t first) {
  const uint32_t N = (uint32_t)labels.size();
  std::vector<uint32_t> start(N + 1, 0), order(N);
  for (uint32_t g = 0; g < N; ++g) start[labels[g] + 1] += 1;
  for (uint32_t g = 0; g < N; ++g) start[g + 1] += start[g];
  std::vector<uint32_t> at(start.begin(), start.end() - 1);
  for (uint32_t g = 0; g < N; ++g) if (labels[g] == g) order[at[g]++] = g;
  for (uint32_t g = 0; g < N; ++g) if (labels[g] != g) order[at[labels[g]]++] = g;
  ParallelTextWriter out(filestr, host_threads());
  std::string text;
  for (uint32_t i = 0; i < N; ++i) {
    const uint32_t g = order[i];
    if (g < first) continue;   // (--novel: the given genomes have no lines)
    text += filenames[labels[g]];
    text += '\t';
    text += filenames[g];
    text += '\n';
    if (text.size() >= (size_t(4) << 20)) { out.write(text); text.clear(); }
  }
  out.write(text);
  out.close();
}

void Index::cluster_to_file(const std::string &filestr) {
  const auto call = NEED(SELF_JOIN, niqki_cluster);
  const uint32_t N = (uint32_t)filenames.size();
  niqki_params p{};
  check(niqki_get_params(h_, &p), "niqki_get_params");
  std::vector<uint32_t> labels(N);
  uint32_t n_clusters = 0;
  check(call(h_, p.min_score, labels.data(), &n_clusters, NIQKI_MEM_HOST), "niqki_cluster");
  // (a label is its cluster's smallest id: label order is index order and the label leads its cluster anyway)
  write_groups(filestr, labels);
}

void Index::dereplicate(const std::string &list_file, const std::string &dump_file) {
  const auto call = NEED(DEREPLICATION, niqki_dereplicate);
  const uint32_t N = (uint32_t)filenames.size();
  niqki_params p{};
  check(niqki_get_params(h_, &p), "niqki_get_params");
  std::vector<uint32_t> labels(N);
  check(call(h_, p.min_score, labels.data(), nullptr, nullptr, NIQKI_MEM_HOST), "niqki_dereplicate");
  // a representative may stand for genomes that precede it in the index: its own line still leads its group
  if (!list_file.empty()) write_groups(list_file, labels);
  if (dump_file.empty()) return;
  std::vector<uint8_t> keep(N);
  for (uint32_t g = 0; g < N; ++g) keep[g] = labels[g] == g;
  retain(keep);
  dump_index_disk(dump_file);
}

void Index::linkage_to_files(const std::string &mst_file, const std::string &linkage_file, const std::string &tree_file) {
  const auto call = NEED(LINKAGE, niqki_linkage);
  const uint32_t N = (uint32_t)filenames.size();
  niqki_params p{};
  check(niqki_get_params(h_, &p), "niqki_get_params");
  std::vector<uint32_t> into(N), count(N), lo(N), hi(N), ec(N);
  uint32_t n_roots = 0;
  const bool edges = !mst_file.empty();
  check(call(h_, p.min_score, into.data(), count.data(), edges ? lo.data() : nullptr, edges ? hi.data() : nullptr,
             edges ? ec.data() : nullptr, &n_roots, NIQKI_MEM_HOST), "niqki_linkage");
  const auto to_file = [&](const std::string &filestr, auto &&writer) {
    if (filestr.empty()) return;
    ParallelTextWriter out(filestr, host_threads());
    writer([&](const std::string &text) { out.write(text); });
    out.close();
  };
  lo.resize(N - n_roots);
  hi.resize(N - n_roots);
  ec.resize(N - n_roots);
  to_file(mst_file, [&](auto &&sink) { write_mst(lo, hi, ec, filenames, F, sink); });
  to_file(linkage_file, [&](auto &&sink) { write_linkage(into, count, filenames, F, sink); });
  to_file(tree_file, [&](auto &&sink) { write_tree(into, count, filenames, F, sink); });
}

// ---- label audit ---------------------------------------------------------------------

const char *const Index::kAuditVerdicts[5] = {"alone", "agrees", "tied", "misplaced", "stray"};
static_assert(NIQKI_AUDIT_ALONE == 0 && NIQKI_AUDIT_AGREES == 1 && NIQKI_AUDIT_TIED == 2 && NIQKI_AUDIT_MISPLACED == 3 &&
                  NIQKI_AUDIT_STRAY == 4,
              "kAuditVerdicts is indexed by the verdict");

std::vector<uint64_t> Index::audit_to_file(const std::string &filestr, uint32_t k, const std::string &label_file, const char *option) {
  const auto set_labels = NEED(AUDIT, niqki_set_labels);
  const auto call = NEED(AUDIT, niqki_audit);
  LabelFile lf;
  read_labels(option, label_file, lf.label_of, lf.texts);
  const uint32_t N = (uint32_t)lf.label_of.size();
  niqki_params p{};
  check(niqki_get_params(h_, &p), "niqki_get_params");
  check(set_labels(h_, N ? lf.label_of.data() : nullptr, N, NIQKI_MEM_HOST), "niqki_set_labels");
  std::vector<uint32_t> verdict(N), own_c(N), own_g(N), oth_c(N), oth_g(N), vote_g(N), vote_n(N);
  check(call(h_, p.min_score, k, verdict.data(), own_c.data(), own_g.data(), oth_c.data(), oth_g.data(), vote_g.data(), vote_n.data(),
             NIQKI_MEM_HOST), "niqki_audit");
  std::vector<uint64_t> totals(5, 0);
  ParallelTextWriter out(filestr, host_threads());
  std::string text;
  // name:jaccard of neighbour g at `count`, "-" where there is none
  const auto neighbour = [&](uint32_t g, uint32_t count) {
    if (g >= N) return std::string("-");
    return filenames[g] + ':' + fmt_double((double)count / F);
  };
  for (uint32_t g = 0; g < N; ++g) {
    if (verdict[g] >= 5) throw std::runtime_error("niqki_audit gave a verdict the program does not know");
    totals[verdict[g]] += 1;
    text += filenames[g];
    text += '\t';
    text += lf.texts[lf.label_of[g]];
    text += '\t';
    text += kAuditVerdicts[verdict[g]];
    text += '\t';
    text += neighbour(own_g[g], own_c[g]);
    text += '\t';
    text += neighbour(oth_g[g], oth_c[g]);
    text += '\t';
    text += oth_g[g] < N ? lf.texts[lf.label_of[oth_g[g]]] : std::string("-");
    text += '\t';
    text += vote_g[g] < N ? lf.texts[lf.label_of[vote_g[g]]] + ':' + std::to_string(vote_n[g]) : std::string("-");
    text += '\n';
    if (text.size() >= (size_t(4) << 20)) { out.write(text); text.clear(); }
  }
  out.write(text);
  out.close();
  return totals;
}

// ---- merging dumps ------------------------------------------------------------------

void Index::merge_dump(const std::string &dump_file) {
  const auto begin = NEED(APPEND, niqki_append_begin);
  const auto slots = NEED(APPEND, niqki_append_slots);
  const auto cancel = NEED(APPEND, niqki_append_cancel);
  std::vector<std::string> names;
  bool pending = false;
  try {
    walk_dump(
        dump_file,
        [&](const uint8_t *hdr) {
          check(begin(h_, hdr), "niqki_append_begin");
          uint32_t n_new;
          std::memcpy(&n_new, hdr + 20, 4);
          pending = n_new != 0;   // (an empty dump is committed by its header)
        },
        [&](uint32_t s0, uint32_t s1, const uint8_t *data, size_t len) {
          if (!pending) return;
          uint64_t used = 0;
          const int rc = slots(h_, s0, s1, data, len, &used);
          if (rc) pending = false;   // (the engine has cancelled the append itself)
          check(rc, "niqki_append_slots");
          if (s1 == F) pending = false;
        },
        names);
  } catch (const std::exception &e) {
    // refused: the index is the one before the merge, and nothing is written, the -O file included
    if (pending) (void)cancel(h_);
    refuse("--merge '" + dump_file + "': " + e.what());
  }
  filenames.insert(filenames.end(), std::make_move_iterator(names.begin()), std::make_move_iterator(names.end()));
}

void Index::keep_novel(uint32_t first, uint32_t threshold, const std::string &list_file) {
  const auto call = NEED(DEREPLICATION_FROM, niqki_dereplicate_from);
  const uint32_t N = (uint32_t)filenames.size();
  std::vector<uint32_t> labels(N);
  check(call(h_, first, threshold, labels.data(), nullptr, nullptr, NIQKI_MEM_HOST), "niqki_dereplicate_from");
  write_groups(list_file, labels, first);
  std::vector<uint8_t> keep(N);
  bool all = true;
  for (uint32_t g = 0; g < N; ++g) all &= (keep[g] = labels[g] == g) != 0;
  if (!all) retain(keep);
}

// ---- dropping genomes ---------------------------------------------------------------

void Index::retain(const std::vector<uint8_t> &keep) {
  const auto call = NEED(RETAIN, niqki_retain);
  if (keep.size() != filenames.size()) throw std::runtime_error("retain: one flag per indexed genome");
  uint32_t n_kept = 0;
  check(call(h_, keep.data(), nullptr, &n_kept, NIQKI_MEM_HOST), "niqki_retain");
  size_t at = 0;
  for (size_t g = 0; g < keep.size(); ++g)
    if (keep[g]) {
      if (at != g) filenames[at] = std::move(filenames[g]);
      ++at;
    }
  filenames.resize(at);
  if (at != n_kept) throw std::runtime_error("niqki_retain kept another number of genomes than asked");
}

void Index::remove_listed(const std::string &filestr) {
  std::ifstream in(filestr);
  if (!in) throw std::runtime_error("--remove: cannot open '" + filestr + "'");
  std::unordered_set<std::string> listed, seen;
  std::vector<std::string> in_order;
  for (std::string line; std::getline(in, line);) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (!line.empty() && listed.insert(line).second) in_order.push_back(line);
  }
  std::vector<uint8_t> keep(filenames.size(), 1);
  for (size_t g = 0; g < filenames.size(); ++g)
    if (listed.count(filenames[g])) { keep[g] = 0; seen.insert(filenames[g]); }
  for (const std::string &name : in_order)
    if (!seen.count(name)) refuse("--remove: no indexed genome is named '" + name + "'");
  if (!listed.empty()) retain(keep);
}

// ---- one entry per label -------------------------------------------------------------

void Index::unite_listed(const std::string &filestr) {
  const auto call = NEED(UNITE, niqki_unite);
  LabelFile lf;
  read_labels("--pan", filestr, lf.label_of, lf.texts);
  const uint32_t N = (uint32_t)lf.label_of.size();
  std::vector<uint32_t> entry_of(N);
  uint32_t n_entries = 0;
  check(call(h_, N ? lf.label_of.data() : nullptr, N, N ? entry_of.data() : nullptr, &n_entries, NIQKI_MEM_HOST), "niqki_unite");
  if (n_entries != lf.texts.size()) throw std::runtime_error("niqki_unite made another number of entries than the file has labels");
  std::vector<std::string> names(n_entries);
  for (uint32_t g = 0; g < N; ++g) names[entry_of[g]] = lf.texts[lf.label_of[g]];
  filenames = std::move(names);
}

// ---- dump ------------------------------------------------------------------------

void Index::dump_index_disk(const std::string &filestr) {
  // header + buckets (src/niqki_index.cpp:42-55) exported in groups of whole slots
  // and gzipped in parallel, then the names (:56-58)
  const bool timing = std::getenv("NIQKI_HOST_TIMING") != nullptr;
  Lap lap;
  double t_layout = 0, t_alloc = 0, t_export = 0, t_writer = 0;
  ParallelGzWriter out(filestr, host_threads() + 1);   // (the CPUs this process may use: its cgroup quota counts)
  {
    std::vector<uint8_t> hdr(24);
    check(niqki_export_dump_header(h_, hdr.data()), "niqki_export_dump_header");
    out.add(hdr);
  }
  const uint64_t target = uint64_t(32) << 20;
  uint64_t payload = 0;
  for (size_t r = 0; r < sh_.size(); ++r) {   // the shards' slots in rank order are the whole payload
    uint32_t sb = 0, se = F;
    if (grp_) niqki_group_slot_range((uint32_t)r, (uint32_t)sh_.size(), lF, &sb, &se);
    const uint32_t f_local = se - sb;
    std::vector<uint64_t> slot_bytes((size_t)f_local + 1);
    check(niqki_export_dump_layout(sh_[r], slot_bytes.data()), "niqki_export_dump_layout");
    lap.to(t_layout);
    uint32_t s0 = 0;
    while (s0 < f_local) {
      uint32_t s1 = s0 + 1;
      while (s1 < f_local && slot_bytes[s1 + 1] - slot_bytes[s0] <= target) ++s1;
      const uint64_t want = slot_bytes[s1] - slot_bytes[s0];
      ParallelGzWriter::Block block(want);
      lap.to(t_alloc);
      uint64_t size = 0;
      check(niqki_export_dump_slots(sh_[r], s0, s1, block.data(), want, &size), "niqki_export_dump_slots");
      lap.to(t_export);
      payload += want;
      out.add(std::move(block));
      lap.to(t_writer);
      s0 = s1;
    }
  }
  std::vector<uint8_t> names;
  for (const auto &nm : filenames) {
    names.insert(names.end(), nm.begin(), nm.end());
    names.push_back('\n');
  }
  out.add(names);
  out.finish();
  lap.to(t_writer);
  if (timing)
    std::cerr << "[niqki timing] dump: " << payload / 1e9 << " GB of buckets: layout " << t_layout << " s, buffers " << t_alloc
              << ", export (kernel + copy) " << t_export << ", waiting for the gzip writer " << t_writer << std::endl;
}

}  // namespace nqhost
