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

  // The self-join (long options --neighbors / --cluster; single-GPU index).  The two engine calls are looked up at run
  // time, so that the program still links against an engine that answers the C ABI without them.
  static bool has_self_join();
  // the indexed genomes as queries, in index order, written like a -Q batch (niqki_neighbors_range)
  void query_neighbors();
  // single-linkage clusters at min_score (niqki_cluster) as lines representative<TAB>member: clusters in the order of
  // their representative's index position, members in index order; a gzip file like every output of the program
  void cluster_to_file(const std::string &filestr);
  // Dereplication (long option --derep; single-GPU index; niqki_dereplicate, looked up at run time like the two above):
  // greedy representatives at min_score in index order, as lines representative<TAB>member: groups in the order of
  // their representative's index position, the representative's own line first, then its members in index order
  static bool has_dereplication();
  void dereplicate_to_file(const std::string &filestr) { dereplicate(filestr, ""); }
  // Dropping genomes (long options --remove / --derep-dump; single-GPU index; niqki_retain, looked up at run time like
  // the calls above).  retain: the genomes with a zero flag leave the engine's index and `filenames`; the rest keep
  // their order.  remove_listed: drops every genome that carries a name of the file (one per line); a name no genome
  // carries is an error, and then nothing is written, the -O file included.
  static bool has_retain();
  void retain(const std::vector<uint8_t> &keep);
  void remove_listed(const std::string &filestr);
  // ONE niqki_dereplicate call for --derep and --derep-dump: the list of the full index into list_file (unless empty),
  // then, unless dump_file is empty, only the representatives are retained and dumped there (dump_index_disk); the
  // index in memory is the dereplicated one from then on
  void dereplicate(const std::string &list_file, const std::string &dump_file);

  // Merging dumps (long option --merge; single-GPU index; niqki_append_begin / _slots / _cancel, looked up at run time
  // like the calls above).  The dump file is streamed through the readers of the loading constructor, whole slots go to
  // the engine's pending append, and its names follow `filenames` (duplicates are kept as they are).  A dump the engine
  // refuses (other lF / K / W / H, a broken payload) leaves the index as it was and is an error, and then nothing is
  // written, the -O file included.
  static bool has_append();
  void merge_dump(const std::string &dump_file);
  // The novelty filter (long option --novel; niqki_dereplicate_from + niqki_retain): the genomes below `first` are
  // given; of the others the representatives at `threshold` (a co-occurrence count, as min_score) stay.  list_file gets the --derep lines of the genomes from
  // `first` on; the index in memory holds the given genomes and the new representatives from then on.
  static bool has_dereplication_from();
  void keep_novel(uint32_t first, uint32_t threshold, const std::string &list_file);

  // The linkage phase (long options --mst / --linkage / --tree; single-GPU index; niqki_linkage, looked up at run time
  // like the calls above): ONE engine call at min_score as the floor serves the three files (an empty name: not
  // written); the texts are linkage_text.h's, gzip files like every output of the program.
  static bool has_linkage();
  void linkage_to_files(const std::string &mst_file, const std::string &linkage_file, const std::string &tree_file);

  // The greedy cover (long option --cover; single-GPU resident index; niqki_staged_cover, looked up at run time like
  // the calls above).  With `cover` set the list of every -Q / -l query is its cover instead of its hits: per pick the
  // genome and the slots it newly explains, at most top_k picks where top_k > 0; --neighbors and -M are not affected.
  static bool has_cover();
  bool cover = false;
  // Collapsed hits (long option --collapse <file>; single-GPU index; niqki_set_labels + niqki_staged_query_collapsed,
  // looked up at run time like the calls above).  set_collapse reads the label file (label_file.h; plain or gzip) against
  // `filenames` as they are at that moment and hands the labels to the engine; from then on the list of every -Q / -l
  // query holds one entry per label -- the label's text and the jaccard of its best member -- at most top_k labels
  // where top_k > 0; --neighbors and -M are not affected.  A file error is an error of the run, and then nothing is
  // written, the -O file included.
  static bool has_collapse();
  void set_collapse(const std::string &filestr);
  // Taxon of a query (long options --lca <file>, --lca-top <permille>; single-GPU index; niqki_set_taxonomy +
  // niqki_staged_query_lca, looked up at run time like the calls above).  set_lca reads the taxonomy file
  // (taxonomy_file.h; plain or gzip) over the label texts of the run -- those of label_file (the --collapse file)
  // where it is not empty, else every genome under its own name -- and hands genome taxa and parents to the engine;
  // from then on the list of every -Q / -l query holds at most one entry, taxonText:jaccard of the best hit
  // ("no_common_taxon" where the considered hits lie in two trees); --neighbors and -M are not affected.  A file error
  // is an error of the run, and then nothing is written, the -O file included.
  static bool has_lca();
  void set_lca(const std::string &filestr, uint32_t top_permille, const std::string &label_file);

  void output_query(const query_output &toprint, const std::string &queryname);   // :544-566
  void output_matrix_row(const uint16_t *counts, const std::string &queryname);   // :747-763

 private:
  void write_groups(const std::string &filestr, const std::vector<uint32_t> &labels, uint32_t first = 0);   // lines of members >= first
  struct Batch;
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
    // lines mode: the names are header lines of a piece of the input that stays alive until the WRITER thread has
    // taken them (name e = the line at name_base + name_at[e]); `keep` is that piece
    const uint8_t *name_base = nullptr;
    size_t name_room = 0;
    std::vector<uint64_t> name_at;
    void *keep = nullptr;
  };
  void query_staged(size_t n, Hits &h);
  void write_hits(const Hits &h);
  bool collapse_ = false;                // --collapse: set_collapse has run
  std::vector<uint32_t> label_of_;      // ... per genome its label, per label its text (label_file.h)
  std::vector<std::string> label_text_;
  bool lca_ = false;                     // --lca: set_lca has run
  uint32_t lca_permille_ = 0;
  std::vector<std::string> taxon_text_;  // ... per taxon its text (taxonomy_file.h)
  std::string out_text_;                // write_hits' lines before they go to the writer
  std::string out_path_;                // the -O file (remove_listed takes it away again when it refuses)
  void stream_lines(const std::string &filestr, bool insert);
  void check(int rc, const char *what) const;
  void check_group(int rc, const char *what) const;
  void make_shards(const niqki_params &p, int device, int n_gpus, const uint8_t *dump_header);
  uint32_t per_rank(size_t n) const { return (uint32_t)((n + sh_.size() - 1) / sh_.size()); }
  // multi-GPU: hits of a batch whose entries sit in the shards' staged batches (n_entry[r] of rank r)
  void group_query_staged(uint32_t per, const std::vector<uint32_t> &n_entry, Hits &h);
  niqki_index *h_ = nullptr;            // shard 0 (the only one with one GPU)
  std::vector<niqki_index *> sh_;       // all shards, rank order
  niqki_group *grp_ = nullptr;          // null with one GPU
  // whole-file queries: where flush_query hands a batch's hits (for_each_batch: a writer thread formats and writes them
  // while the next batch is on the GPU); empty: written on the spot
  std::function<void(std::unique_ptr<Hits>)> hits_sink_;
  double t_stage_ = 0, t_dev_ = 0, t_out_ = 0;  // NIQKI_HOST_TIMING: copy + frame / sketch + insert or query / output text
};

}  // namespace nqhost
