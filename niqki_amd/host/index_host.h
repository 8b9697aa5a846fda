// index_host.h -- host-side mirror of the reference's Index class
// (src/niqki_index.h:35-213) for the file-level drivers: same method names and
// argument meaning, the per-record work (compute_sketch / insert_sketch /
// query_sketch) batched through the C ABI of libniqki_hip.so.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/niqki_hip.h"
#include "gzio.h"
#include "size_estimate.h"

namespace nqhost {

using query_output = std::vector<std::pair<uint32_t, uint32_t>>;  // (count, gid), src/niqki_index.h:31

class Index {
 public:
  // Index(lF,K,W,H,filename,min_fract): src/niqki_index.cpp:13-38
  // n_gpus > 1 (the program's --gpus): the index is cut by sketch-slot range over devices
  // device .. device + n_gpus - 1 (niqki_group_*, RCCL inside libniqki_hip.so); the files of a
  // batch are dealt to the GPUs in order, every GPU frames and sketches its share
  // resident_mib > 0 (the program's --resident-mib): a paged index -- the sketch store in page-locked host
  // memory, the inverted index built for one page of slots at a time within that budget
  // top_k > 0 (the program's --top): a query reports the first top_k entries of its list (niqki_params.top_k)
  Index(uint32_t lF, uint32_t K, uint32_t W, uint32_t H, const std::string &out_filename, double min_fract,
        int device = -1, int n_gpus = 1, int resident_mib = 0, uint32_t top_k = 0);
  // Index(dump file, pretty, filename): src/niqki_index.cpp:63-102
  Index(const std::string &dump_file, bool pretty_printing, const std::string &out_filename, int device = -1,
        int n_gpus = 1, int resident_mib = 0, uint32_t top_k = 0);
  ~Index();
  Index(const Index &) = delete;
  Index &operator=(const Index &) = delete;

  uint32_t K = 0, W = 0, H = 0, lF = 0, F = 0, min_score = 0, top_k = 0;
  bool pretty_printing = true;
  std::vector<std::string> filenames;
  std::unique_ptr<ParallelTextWriter> outfile;

  size_t getNbGenomes() const { return filenames.size(); }  // src/niqki_index.h:138-140

  void select_best_H(double genome_size);  // src/niqki_index.cpp:126-138 (-G)

  // per-record operators, kept for API parity (src/niqki_index.h:103,108,142)
  void compute_sketch(const std::string &reference, std::vector<int32_t> &sketch) const;
  void insert_sketch(const std::vector<int32_t> &sketch, uint32_t genome_id);
  query_output query_sketch(const std::vector<int32_t> &sketch) const;

  // file drivers
  void insert_file_of_file_whole(const std::string &filestr);  // :461-500
  void insert_file_lines(const std::string &filestr);          // :383-408
  void query_file_of_file_whole(const std::string &filestr);   // :523-540
  void query_file_lines(const std::string &filestr);           // :412-430
  void query_matrix();                                          // :614-628
  void dump_index_disk(const std::string &filestr);            // :42-59

  // What an engine may answer the C ABI without (the CPU stand-in of the test suite is such an engine): the calls behind
  // the long options below are looked up at run time, so the program links against any engine, and a run that needs one
  // the engine lacks is refused with the feature's text.  One table in index_host.cpp holds, per feature, the symbols it
  // needs and that text.  All of these work on a single-GPU index only.
  enum class Feature { APPEND, DEREPLICATION_FROM, RETAIN, UNITE, SELF_JOIN, DEREPLICATION, LINKAGE, AUDIT, LCA, COVER, SIZES, CONTAINED, COLLAPSE, TALLY };
  // null where the engine has every call of the feature, else the text that says what is missing
  static const char *lacks(Feature f);

  // --neighbors: the indexed genomes as queries, in index order, written like a -Q batch (niqki_neighbors_range)
  void query_neighbors();
  // --cluster: single-linkage clusters at min_score (niqki_cluster) as lines representative<TAB>member: clusters in the
  // order of their representative's index position, members in index order; a gzip file like every output of the program
  void cluster_to_file(const std::string &filestr);
  // --derep / --derep-dump, ONE niqki_dereplicate call for both: greedy representatives at min_score in index order.
  // list_file (unless empty) gets lines representative<TAB>member of the full index: groups in the order of their
  // representative's index position, the representative's own line first, then its members in index order.  Then, unless
  // dump_file is empty, only the representatives are retained and dumped there (dump_index_disk); the index in memory
  // is the dereplicated one from then on.
  void dereplicate(const std::string &list_file, const std::string &dump_file);
  void dereplicate_to_file(const std::string &filestr) { dereplicate(filestr, ""); }
  // --remove (niqki_retain).  retain: the genomes with a zero flag leave the engine's index and `filenames`; the rest
  // keep their order.  remove_listed: drops every genome that carries a name of the file (one per line); a name no
  // genome carries is an error, and then nothing is written, the -O file included.
  void retain(const std::vector<uint8_t> &keep);
  void remove_listed(const std::string &filestr);
  // --pan <file> (niqki_unite).  Reads the label file (label_file.h; plain or gzip, the format and the rules of
  // --collapse) against `filenames`; the engine's index then holds one entry per label, its sketch the union of the
  // members' sketches, and `filenames` the label texts in entry order.  A file error is an error of the run, and then
  // nothing is written, the -O file included.
  void unite_listed(const std::string &filestr);
  // --merge (niqki_append_begin / _slots / _cancel).  The dump file is streamed through the readers of the loading
  // constructor, whole slots go to the engine's pending append, and its names follow `filenames` (duplicates are kept as
  // they are).  A dump the engine refuses (other lF / K / W / H, a broken payload) leaves the index as it was and is an
  // error, and then nothing is written, the -O file included.
  void merge_dump(const std::string &dump_file);
  // --novel (niqki_dereplicate_from + niqki_retain): the genomes below `first` are given; of the others the
  // representatives at `threshold` (a co-occurrence count, as min_score) stay.  list_file gets the --derep lines of the
  // genomes from `first` on; the index in memory holds the given genomes and the new representatives from then on.
  void keep_novel(uint32_t first, uint32_t threshold, const std::string &list_file);
  // --mst / --linkage / --tree: ONE niqki_linkage call at min_score as the floor serves the three files (an empty name:
  // not written); the texts are linkage_text.h's, gzip files like every output of the program.
  void linkage_to_files(const std::string &mst_file, const std::string &linkage_file, const std::string &tree_file);
  // --audit <file>, --audit-k <n> (niqki_set_labels + niqki_audit at min_score).  Reads the run's label file
  // (label_file.h; `option` is --pan or --collapse, whichever supplied it) against `filenames` as they are at that
  // moment, hands the labels to the engine and writes a line per indexed genome, in index order, a gzip file like every
  // output of the program:
  //   name<TAB>label<TAB>verdict<TAB>ownName:jaccard<TAB>otherName:jaccard<TAB>otherLabel<TAB>voteLabel:votes
  // the nearest other genome under the genome's label, the nearest under another label and that label, the label most
  // frequent among the k nearest; "-" where there is no such neighbour; verdict as the engine gives it.  Returns the
  // number of genomes per verdict.  A file error is an error of the run, and then nothing is written, the -O file
  // included.
  std::vector<uint64_t> audit_to_file(const std::string &filestr, uint32_t k, const std::string &label_file, const char *option);
  static const char *const kAuditVerdicts[5];   // the texts of NIQKI_AUDIT_ALONE .. NIQKI_AUDIT_STRAY

  // The three that replace the list of every -Q / -l query; --neighbors and -M are not affected.
  // --cover (niqki_staged_cover; resident index): with `cover` set the list is the query's greedy cover: per pick the
  // genome and the slots it newly explains, at most top_k picks where top_k > 0.
  bool cover = false;
  // --collapse <file> (niqki_set_labels + niqki_staged_query_collapsed).  set_collapse reads the label file
  // (label_file.h; plain or gzip) against `filenames` as they are at that moment and hands the labels to the engine;
  // from then on the list holds one entry per label -- the label's text and the jaccard of its best member -- at most
  // top_k labels where top_k > 0.  A file error is an error of the run, and then nothing is written, the -O file included.
  void set_collapse(const std::string &filestr);
  // --lca <file>, --lca-top <permille> (niqki_set_taxonomy + niqki_staged_query_lca).  set_lca reads the taxonomy file
  // (taxonomy_file.h; plain or gzip) over the label texts of the run -- those of label_file (the --collapse file)
  // where it is not empty, else every genome under its own name -- and hands genome taxa and parents to the engine;
  // from then on the list holds at most one entry, taxonText:jaccard of the best hit ("no_common_taxon" where the
  // considered hits lie in two trees).  A file error is an error of the run, and then nothing is written, the -O file
  // included.
  void set_lca(const std::string &filestr, uint32_t top_permille, const std::string &label_file);
  // --report <file> beside --lca (niqki_tally_begin + niqki_tally_read).  With `report` set, set_lca opens the engine's
  // taxon tally, which every -Q / -l query of the run then feeds; write_report reads it once, after the last of them,
  // and writes report_file.h's text into `report`, a gzip file like every output of the program.  --neighbors and -M
  // are not tallied.
  std::string report;
  void write_report();

  // --sizes <file> (niqki_registers + size_estimate.h): a line per indexed genome, in index order, a gzip file like
  // every output of the program: name<TAB>kmers<TAB>status -- the estimated number of distinct k-mers (%.0f) and ok,
  // below or above (outside the estimator's range: the number is not to be used).
  void sizes_to_file(const std::string &filestr);
  // --containment (niqki_registers once, niqki_staged_registers per batch): with `containment` set every entry of a
  // plain -Q / -l list is name:jaccard:cq:cg -- the share of the query's k-mers found in the genome and of the genome's
  // found in the query, "-" each where either size is not ok.  Order, threshold and --top are those of the plain list.
  bool containment = false;
  // --min-containment <x>, --containment-of query|genome|either (niqki_set_sizes once + niqki_staged_query_contained):
  // with min_share > 0 the entries of a -Q / -l list are those whose containment reaches x, ordered by it and cut to
  // top_k on the device, in --containment's format.  The integer sizes are floor(estimate + 0.5) where the status is ok,
  // else 0 (such a hit is never listed); min_score stays the floor.  unsized_hits: the hits of all queries so far that
  // had no size estimate.
  uint32_t min_share = 0, contain_mode = 0;
  uint64_t unsized_hits = 0;

  void output_query(const query_output &toprint, const std::string &queryname);   // :544-566
  void output_matrix_row(const uint16_t *counts, const std::string &queryname);   // :747-763

 private:
  void write_groups(const std::string &filestr, const std::vector<uint32_t> &labels, uint32_t first = 0);   // lines of members >= first
  // the feature's call `name` as an Fn; throws the feature's text where the engine lacks it or the index is a --gpus group
  template <typename Fn>
  Fn need(Feature f, const char *name) const;
  // a run refused before anything is written: the output file the constructor made goes away again, `text` is thrown
  [[noreturn]] void refuse(const std::string &text);
  // the label file of `option` (--collapse, --pan; label_file.h, plain or gzip) read against `filenames`: per genome its
  // label, per label its text; a file error refuses the run with the option, the file and the line
  void read_labels(const char *option, const std::string &filestr, std::vector<uint32_t> &label_of, std::vector<std::string> &texts);
  void open_group_and_output(const std::string &out_filename);   // the tail of both constructors
  struct Batch;
  // The entries of a batch dealt to the GPUs in order: n_entry[r] of them on rank r, at most `per` on any (one GPU:
  // all of them on rank 0).
  struct Share {
    uint32_t per = 0;
    std::vector<uint32_t> n_entry;
  };
  Share rank_share(size_t n) const;   // whole-file mode: n files, ceil(n / GPUs) to each rank in list order
  void stage_batch(Batch &b, bool prefetch);
  void flush_insert(Batch &b);
  void flush_query(Batch &b);
  void for_each_batch(const std::vector<std::string> &paths, void (Index::*flush)(Batch &));
  struct Hits {  // hits of a batch of entries: (count, gid) runs hc/hg[off[i] .. off[i+1]) for names[i]
    std::vector<std::string> names;
    std::vector<uint64_t> off;
    std::vector<uint32_t> hc, hg;
    bool collapsed = false;   // hg names each label's best member: the line prints the label's text (--collapse)
    bool lca = false;         // hg holds a taxon (NIQKI_TAXON_NONE: no common one): the line prints the taxon's text (--lca)
    std::vector<nqsize::Estimate> qsize;   // --containment: the entries' sizes (empty: a plain list)
    // lines mode: the names are header lines of a piece of the input that stays alive until the WRITER thread has
    // taken them (name e = the line at name_base + name_at[e]); `keep` is that piece
    const uint8_t *name_base = nullptr;
    size_t name_room = 0;
    std::vector<uint64_t> name_at;
    void *keep = nullptr;
  };
  struct HitsWriter;   // the thread that formats and writes a batch's hits while the next batch is on the GPU
  // the staged entries of `s`: inserted / their hits, in entry order (rank after rank)
  void staged_insert(const Share &s);
  void staged_hits(const Share &s, Hits &h);
  void query_staged(size_t n, Hits &h);                    // ... one GPU
  void group_query_staged(const Share &s, Hits &h);       // ... the shards of a group
  void write_hits(const Hits &h);
  bool collapse_ = false;                // --collapse: set_collapse has run
  std::vector<uint32_t> label_of_;      // ... per genome its label, per label its text (label_file.h)
  std::vector<std::string> label_text_;
  bool lca_ = false;                     // --lca: set_lca has run
  uint32_t lca_permille_ = 0;
  std::vector<std::string> taxon_text_;  // ... per taxon its text (taxonomy_file.h)
  std::vector<uint32_t> taxon_parent_;   // ... and its parent (--report)
  bool tally_open_ = false;              // --report: the engine's tally is open (an index without genomes has no taxonomy to open it on)
  uint64_t untallied_ = 0;               // ... else the entries queried: none of them has a hit
  // the sizes of the indexed genomes [0, n) from their register histograms (niqki_registers, size_estimate.h)
  std::vector<nqsize::Estimate> genome_sizes(uint32_t n) const;
  std::vector<nqsize::Estimate> genome_size_;   // --containment: ... taken once, at the first query batch
  bool genome_size_ok_ = false;
  // ... and the sizes of the n staged entries into h.qsize, from their staged sketches (niqki_staged_registers)
  void staged_sizes(size_t n, uint32_t N, Hits &h);
  bool sizes_set_ = false;              // --min-containment: niqki_set_sizes has run
  std::string out_text_;                // write_hits' lines before they go to the writer
  std::string out_path_;                // the -O file (refuse takes it away again)
  // Lines mode.  stage_lines: one niqki_stage_raw of the whole records at raw[0, size) on h -- at most hdr.size()
  // entries, hdr gets the offsets of their header lines.  deal_lines: the same for all GPUs -- the bytes are cut into one
  // run of whole records per GPU, the entries keep the order of the file; `s` gets the entries per rank, name_at their
  // header lines' offsets from raw; returns the bytes taken (less than size: a call took all the entries it may).
  niqki_stage_info stage_lines(niqki_index *h, const uint8_t *raw, size_t size, char type, std::vector<uint64_t> &hdr);
  size_t deal_lines(const uint8_t *raw, size_t size, char type, std::vector<uint64_t> &hdr, Share &s, std::vector<uint64_t> &name_at);
  void stream_lines(const std::string &filestr, bool insert);
  static void check_on(niqki_index *h, int rc, const char *what);
  void check(int rc, const char *what) const { check_on(h_, rc, what); }
  void check_group(int rc, const char *what) const;
  void make_shards(const niqki_params &p, int device, int n_gpus, const uint8_t *dump_header);
  niqki_index *h_ = nullptr;            // shard 0 (the only one with one GPU)
  std::vector<niqki_index *> sh_;       // all shards, rank order
  niqki_group *grp_ = nullptr;          // null with one GPU
  HitsWriter *writer_ = nullptr;        // whole-file queries: where flush_query hands a batch's hits (for_each_batch)
  double t_stage_ = 0, t_dev_ = 0, t_out_ = 0;  // NIQKI_HOST_TIMING: copy + frame / sketch + insert or query / output text
};

}  // namespace nqhost
