// niqki_main.cpp -- the `niqki` command line on the MI355X engine.  Same options, output
// files, info box text and exit codes as the reference's program (behaviour of
// src/niqki.cpp:229-456, option table :102-185); here the run is a table of phases -- index
// inputs, dump, matrix, query inputs -- each a driver of nqhost::Index -> libniqki_hip.so.  Extensions (long options only):
//   --device <n>   HIP device ordinal (default: current device)
//   --gpus <n>     cut the index by sketch-slot range over n GPUs (devices --device .. +n-1)
//   --resident-mib <n>  paged index: sketch store in host memory, n MiB of device memory for one page of slots
//   --top <n>      report at most n best hits per query (-Q / -q; niqki_params.top_k), 0 = all
//   --neighbors    the indexed genomes themselves as queries, in index order, written like -Q (niqki_neighbors_range)
//   --cover        the list of every -Q / -q query is its greedy cover (niqki_staged_cover): the genome that explains
//                  the most query slots, then the one that explains the most of the rest, ...; --top bounds the picks
//   --collapse <f> f holds lines label<TAB>member (what --cluster / --derep write, or a taxonomy table): the list of
//                  every -Q / -q query holds one entry per label, label:jaccard of the label's best member
//                  (niqki_set_labels + niqki_staged_query_collapsed); --top bounds the labels
//   --lca <f>      f holds lines parent<TAB>child over taxon texts whose leaves are the labels of --collapse or, without
//                  it, the genome names: the list of every -Q / -q query holds one entry, taxon:jaccard, the lowest taxon
//                  that contains every hit within --lca-top permille (default 100) of the best hit, and the best hit's
//                  jaccard (niqki_set_taxonomy + niqki_staged_query_lca); "no_common_taxon" where there is none
//   --report <f>   with --lca: after the last -Q / -l query the taxon tally of all of them into f, a line per taxon with
//                  the queries in its clade and on the taxon itself (niqki_tally_begin + niqki_tally_read; report_file.h)
//   --cluster <f>  single-linkage clusters at the -J threshold into f: representative<TAB>member (niqki_cluster)
//   --mst <f> / --linkage <f> / --tree <f>   the complete single-linkage hierarchy down to the -J threshold from ONE
//                  engine call (niqki_linkage): the maximum spanning forest, the merge table, Newick dendrograms
//   --derep <f>    greedy representatives at the -J threshold, in index order, into f: representative<TAB>member
//                  (niqki_dereplicate); the lines whose two names are equal are the dereplicated list
//   --remove <f>   drop every indexed genome named in f (one name per line) before -D and the queries (niqki_retain)
//   --pan <f>      f holds lines label<TAB>member, as for --collapse: after every index input, --merge, --novel and
//                  --remove the index holds one entry per label, named by the label, whose sketch is the union of the
//                  members' sketches (niqki_unite); -D, the self-join options, -M and the queries see that index
//   --audit <f>    with --pan or --collapse: the leave-one-out neighbours of every indexed genome at the -J threshold read
//                  against that label file, into f (niqki_set_labels + niqki_audit): name, label, verdict (alone, agrees,
//                  tied, misplaced, stray), the nearest other genome under the label, the nearest under another label
//                  and that label, the label most frequent among the --audit-k (default 1) nearest; with --pan the
//                  audit runs immediately before the index is united, with --collapse where that file is applied
//   --derep-dump <f>  dereplicate at the -J threshold, keep the representatives only and dump that index into f (as -D);
//                  the rest of the run (-M, --neighbors, -Q, -l) is answered by the dereplicated index
//   --sizes <f>    after everything that changes the index in memory and before the queries: a line per indexed genome into
//                  f, name<TAB>kmers<TAB>status -- its number of distinct k-mers estimated from the HyperLogLog registers in
//                  the top H bits of its sketch cells (niqki_registers, size_estimate.h), and ok, below or above: outside
//                  the estimator's range the number is not to be used
//   --containment  every entry of a plain -Q / -l list is name:jaccard:cq:cg, the share of the query's k-mers found in the
//                  genome and of the genome's found in the query, from the count and the two estimated sizes
//                  (niqki_staged_registers per batch); -:- where either size is out of range
//   --min-containment <x>  0 < x <= 1: the entries of a -Q / -l list are the hits whose containment reaches x, ordered by it
//                  and cut by --top on the device (niqki_set_sizes + niqki_staged_query_contained), in --containment's
//                  format; -J stays the floor -- a genome below it is never seen, so lower -J to what the smallest share of
//                  interest needs; hits without a size estimate are never listed and are counted on a line of their own
//   --containment-of query|genome|either  with --min-containment: the share is that of the query's k-mers found in the
//                  genome (the default), of the genome's found in the query, or the larger of the two
//   --merge <f>    append the genomes of the dump f to the index (niqki_append_*); may be repeated, ALL occurrences are
//                  taken, in command-line order, after -L / -I / -i and before --remove and -D
//   --novel <f>    after every index input and merge: dereplicate at the -J threshold with the genomes of -L given
//                  (niqki_dereplicate_from), write representative<TAB>member of the other genomes into f and keep only
//                  the representatives among them: -L db.dump --merge delta.dump --novel added.txt -J 0.9 -D db2.dump
#include <libgen.h>
#include <limits.h>
#include <unistd.h>
#include <fcntl.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "index_host.h"

using namespace std;
using namespace std::chrono;

namespace {

enum Opt { LIST, QUERY, LISTLINES, QUERYLINES, KMER, FETCH, OUTPUT, MIN, PRETTY, MATRIX, WORD, GENOME_SIZE, HHL,
           DUMP, LOAD, DOWNLAD, LOGO, HELP, DEVICE, GPUS, RESIDENT, TOP, NEIGHBORS, CLUSTER, DEREP, REMOVE, PAN, DEREP_DUMP, MERGE, NOVEL, MST, LINKAGE, TREE, COVER, COLLAPSE, LCA, LCA_TOP, REPORT, AUDIT, AUDIT_K, SIZES, CONTAINMENT, MIN_CONTAINMENT, CONTAINMENT_OF, N_OPT };
enum ArgKind { NONE, NONEMPTY, NUMERIC };

// Same order as the reference's descriptor table: a short option character
// selects the FIRST entry whose short-option string contains it
// (src/optionparser.h:1654), so -d -> indexdownload, -l -> querylines.
struct Desc { Opt id; const char *shorts; const char *longname; ArgKind kind; const char *help; };
const Desc kDesc[] = {
    {LIST, "I", "index", NONEMPTY, "  --index, -I <filename>        Input file of files to Index."},
    {QUERY, "Q", "query", NONEMPTY, "  --query, -Q <filename>        Input file of file to Query."},
    {LISTLINES, "i", "indexlines", NONEMPTY, "  --indexlines, -i <filename>   Query fa/fq file where each line is a separate entry to Index"},
    {QUERYLINES, "l", "querylines", NONEMPTY, "  --querylines, -q <filename>   Input fa/fq where each line is a separate entry to Query"},
    {KMER, "K", "kmer", NUMERIC, "  --kmer, -K <int>              Kmer size (31)."},
    {FETCH, "S", "sketch", NUMERIC, "  --sketch, -S <int>            Set sketch size to 2^S (15)."},
    {OUTPUT, "O", "output", NONEMPTY, "  --output, -O <filename>       Output file (niqkiOutput.gz)"},
    {MIN, "J", "minjac", NONEMPTY, "  --minjac, -J <int>            Minimal jaccard Index to report (0.1)."},
    {PRETTY, "P", "pretty", NONE, "  --pretty, -P                  Print a human-readable outfile. By default the outfile is in binary."},
    {MATRIX, "M", "matrix", NONEMPTY, "  --matrix, -M <filename>       Output the matrix distance to the given file."},
    {WORD, "W", "word", NUMERIC, "  --word, -W <int>              Fingerprint size (12)."},
    {GENOME_SIZE, "G", "Genomes_sizes", NUMERIC, "  --Genomes_sizes, -G <int>     Rought expectation of the genome sizes."},
    {HHL, "H", "HHL", NUMERIC, "  --HHL, -H <int>               Size of the hyperloglog section (4)."},
    {DUMP, "D", "dump", NONEMPTY, "  --dump, -D <filename>         Dump the current index to the given file."},
    {LOAD, "L", "load", NONEMPTY, "  --load, -L <filename>         Load an index to the given file."},
    {DOWNLAD, "Iddl", "indexdownload", NONEMPTY, "  --indexdownload, -Iddl <filename>  NCBI download (not available in this build)."},
    {LOGO, "", "logo", NONE, "  --logo                        Print ASCII art logo, then exit."},
    {HELP, "h", "help", NONE, "  --help, -h                    Print usage and exit."},
    {DEVICE, "", "device", NUMERIC, "  --device <int>                HIP device ordinal."},
    {GPUS, "", "gpus", NUMERIC, "  --gpus <int>                  Number of GPUs the index is sharded over (1)."},
    {RESIDENT, "", "resident-mib", NUMERIC, "  --resident-mib <int>          Device memory budget of a paged index in MiB (0: everything resident)."},
    {TOP, "", "top", NUMERIC, "  --top <int>                   Report at most <int> best hits per query (0: all)."},
    {NEIGHBORS, "", "neighbors", NONE, "  --neighbors                   Query the index with its own genomes, in index order (output as -Q)."},
    {CLUSTER, "", "cluster", NONEMPTY, "  --cluster <filename>          Single-linkage clusters at the -J threshold: lines representative<TAB>member."},
    {DEREP, "", "derep", NONEMPTY, "  --derep <filename>            Dereplication at the -J threshold: greedy representatives in index order, lines representative<TAB>member."},
    {REMOVE, "", "remove", NONEMPTY, "  --remove <filename>           Drop the indexed genomes named in the file (one name per line) before -D and the queries."},
    {PAN, "", "pan", NONEMPTY, "  --pan <filename>              Unite the indexed genomes by label before -D and the queries: the file holds lines label<TAB>member (as for --collapse); the index then holds one entry per label, named by the label."},
    {DEREP_DUMP, "", "derep-dump", NONEMPTY, "  --derep-dump <filename>       Dereplicate at the -J threshold and dump the index of the representatives (as -D); the rest of the run is answered by that index."},
    {MERGE, "", "merge", NONEMPTY, "  --merge <filename>            Append the genomes of a dump to the index, after -L / -I / -i; may be repeated: every occurrence is taken, in order (of all other options only the last one counts)."},
    {NOVEL, "", "novel", NONEMPTY, "  --novel <filename>            After all index inputs and merges: of the genomes behind those of -L keep only the representatives at the -J threshold (the -L genomes are given); lines representative<TAB>member."},
    {MST, "", "mst", NONEMPTY, "  --mst <filename>              Maximum spanning forest of the index down to the -J threshold: lines nameLo<TAB>nameHi<TAB>jaccard, best edge first."},
    {LINKAGE, "", "linkage", NONEMPTY, "  --linkage <filename>          Single-linkage hierarchy down to the -J threshold: lines name<TAB>merges into<TAB>jaccard (cut it at any threshold for the --cluster groups)."},
    {TREE, "", "tree", NONEMPTY, "  --tree <filename>             Single-linkage dendrograms down to the -J threshold in Newick, one tree per line."},
    {COVER, "", "cover", NONE, "  --cover                       Report each -Q / -q query's greedy cover instead of all its hits: per genome the slots no earlier line explains (--top bounds the picks)."},
    {COLLAPSE, "", "collapse", NONEMPTY, "  --collapse <filename>         Report each -Q / -q query's best hit per label instead of all its hits: the file holds lines label<TAB>member (as --cluster / --derep write them; plain or gzip), a genome no line names is its own label (--top bounds the labels)."},
    {LCA, "", "lca", NONEMPTY, "  --lca <filename>              Report each -Q / -q query's taxon instead of all its hits: the lowest common ancestor of its near-best hits in the taxonomy of the file, lines parent<TAB>child (plain or gzip) over the labels of --collapse or, without it, the genome names; no_common_taxon where the hits share none."},
    {LCA_TOP, "", "lca-top", NONEMPTY, "  --lca-top <permille>          With --lca: consider the hits within <permille> thousandths of the best hit's count, 0..1000 (100); 0: only ties with the best hit."},
    {REPORT, "", "report", NONEMPTY, "  --report <filename>           With --lca: after the last -Q / -l query, the tally of all their taxa: lines percent<TAB>queries in the clade<TAB>queries on the taxon<TAB>depth<TAB>mean jaccard of their best hits<TAB>taxon, indented by depth, after the two lines unclassified and no_common_taxon."},
    {AUDIT, "", "audit", NONEMPTY, "  --audit <filename>            With --pan or --collapse: check that label file against the index at the -J threshold, a line per indexed genome: name<TAB>label<TAB>verdict<TAB>ownName:jaccard<TAB>otherName:jaccard<TAB>otherLabel<TAB>voteLabel:votes (its nearest other genome under its label, the nearest under another label, the vote of its nearest genomes; - where there is none); verdict is alone, agrees, tied, misplaced or stray."},
    {AUDIT_K, "", "audit-k", NONEMPTY, "  --audit-k <n>                 With --audit: the nearest genomes that vote, 1..63 (1)."},
    {SIZES, "", "sizes", NONEMPTY, "  --sizes <filename>            Estimated number of distinct k-mers of every indexed genome, after everything that changes the index and before the queries: lines name<TAB>kmers<TAB>status; status is ok, below or above (outside the estimator's range: do not use the number)."},
    {CONTAINMENT, "", "containment", NONE, "  --containment                 Report each -Q / -q hit as name:jaccard:cq:cg, the share of the query's k-mers found in the genome and of the genome's found in the query (-:- where a size cannot be estimated)."},
    {MIN_CONTAINMENT, "", "min-containment", NONEMPTY, "  --min-containment <x>         Report the -Q / -q hits whose containment reaches x (0 < x <= 1), ordered by it, as name:jaccard:cq:cg (--top cuts that list); -J stays the floor: a genome below it is never seen, so lower -J to what the smallest share of interest needs."},
    {CONTAINMENT_OF, "", "containment-of", NONEMPTY, "  --containment-of <which>      With --min-containment: query (the share of the query's k-mers found in the genome; the default), genome (of the genome's found in the query) or either (the larger of the two)."},
};

struct Parsed {
  bool error = false;
  map<int, vector<string>> opts;  // id -> args in order of appearance ("" for flag options)
  vector<string> non_options;
  bool has(Opt o) const { return opts.count(o) != 0; }
  const string &last(Opt o) const { return opts.at(o).back(); }
};

bool check_arg(const Desc &d, const char *arg, const string &shown) {
  if (d.kind == NONEMPTY) {
    if (arg && arg[0]) return true;
    fprintf(stderr, "Option '%s' requires a non-empty argument\n", shown.c_str());
    return false;
  }
  if (d.kind == NUMERIC) {
    char *end = nullptr;
    if (arg) (void)strtol(arg, &end, 10);
    if (arg && end != arg && *end == 0) return true;
    fprintf(stderr, "Option '%s' requires a numeric argument\n", shown.c_str());
    return false;
  }
  return true;
}

Parsed parse(int argc, char **argv) {
  Parsed p;
  int i = 0;
  for (; i < argc; ++i) {
    const char *a = argv[i];
    if (a[0] != '-' || a[1] == 0) break;            // first non-option ends option parsing (POSIX mode)
    if (a[1] == '-' && a[2] == 0) { ++i; break; }   // "--"
    if (a[1] == '-') {                              // long option
      string name = a + 2, val;
      bool attached = false;
      size_t eq = name.find('=');
      if (eq != string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); attached = true; }
      const Desc *d = nullptr;
      for (const auto &x : kDesc) if (name == x.longname) { d = &x; break; }
      if (!d) { fprintf(stderr, "Unknown option '%s'\n", name.c_str()); p.error = true; return p; }
      if (d->kind == NONE) { p.opts[d->id].push_back(""); continue; }
      const char *arg = attached ? val.c_str() : (i + 1 < argc ? argv[i + 1] : nullptr);
      if (!check_arg(*d, arg, name)) { p.error = true; return p; }
      p.opts[d->id].push_back(arg);
      if (!attached) ++i;
      continue;
    }
    for (const char *c = a + 1; *c; ++c) {          // short option group
      const Desc *d = nullptr;
      for (const auto &x : kDesc) if (x.shorts[0] && strchr(x.shorts, *c)) { d = &x; break; }
      string shown(1, *c);
      if (!d) { fprintf(stderr, "Unknown option '%s'\n", shown.c_str()); p.error = true; return p; }
      if (d->kind == NONE) { p.opts[d->id].push_back(""); continue; }
      const bool attached = c[1] != 0;
      const char *arg = attached ? c + 1 : (i + 1 < argc ? argv[i + 1] : nullptr);
      if (!check_arg(*d, arg, shown)) { p.error = true; return p; }
      p.opts[d->id].push_back(arg);
      if (!attached) ++i;
      break;  // the argument swallowed the rest of the group
    }
  }
  for (; i < argc; ++i) p.non_options.push_back(argv[i]);
  return p;
}

void print_usage() {
  clog << "\n***Input***\n";
  for (const auto &d : kDesc) {
    if (d.id == KMER) clog << "\n***Main parameters***\n";
    if (d.id == OUTPUT) clog << "\n***Output***\n";
    if (d.id == WORD) clog << "\n***Advanced parameters*** (You know what you are doing)\n";
    if (d.id == DUMP) clog << "\n***Index files***\n";
    if (d.id == DOWNLAD) clog << "\n***Other***\n";
    clog << d.help << "\n";
  }
}

// The names inside a file of files are relative to the list: while such a list is read the process
// sits in the list's directory (what src/niqki.cpp:200-224 does around its index and matrix phases).
class ListDir {
 public:
  explicit ListDir(const string &list_path) : back_(open(".", O_CLOEXEC)) {
    vector<char> path(list_path.begin(), list_path.end());
    path.push_back('\0');
    errno = 0;
    if (chdir(dirname(path.data())) != 0) cout << "Error: " << strerror(errno) << endl;
  }
  ~ListDir() {
    errno = 0;
    if (fchdir(back_) != 0) cout << "Error: " << strerror(errno) << endl;
    if (back_ >= 0) close(back_);
  }
  ListDir(const ListDir &) = delete;
  ListDir &operator=(const ListDir &) = delete;

 private:
  int back_;
};

string leaf_of(const string &path) { return path.substr(path.find_last_of("/\\") + 1); }

void warn_if_unreadable(const string &path) {
  if (!ifstream(path)) cout << "Unable to open the file '" << path << "'" << endl;
}

// the three time stamps behind the info box's "lasted" rows
struct RunClock {
  using tp = time_point<system_clock>;
  tp run_begin = system_clock::now(), index_end = run_begin;
  static void row(const char *label, tp from, tp to) {
    cout << label << setw(30) << setfill(' ') << duration<double>(to - from).count() << " |" << endl;
  }
  void index_done() {
    index_end = system_clock::now();
    row("| Indexing lasted (s)               |", run_begin, index_end);
  }
};

template <typename T>
void box_row(const char *label, const T &value) {
  cout << label << setw(30) << setfill(' ') << value << " |" << endl;
}

// One input option = one phase: which Index driver takes the file, and whether it is a list whose
// entries are relative to its own directory.
struct Phase {
  Opt opt;
  bool in_list_dir;
  void (nqhost::Index::*driver)(const string &);
};
const Phase kIndexPhases[] = {{LIST, true, &nqhost::Index::insert_file_of_file_whole},
                              {LISTLINES, true, &nqhost::Index::insert_file_lines}};
const Phase kQueryPhases[] = {{QUERY, false, &nqhost::Index::query_file_of_file_whole},
                              {QUERYLINES, false, &nqhost::Index::query_file_lines}};

void run_phase(nqhost::Index &ix, const Parsed &o, const Phase &ph) {
  if (!o.has(ph.opt)) return;
  const string path = o.last(ph.opt);
  warn_if_unreadable(path);
  if (ph.in_list_dir) {
    ListDir here(path);
    (ix.*ph.driver)(leaf_of(path));
  } else {
    (ix.*ph.driver)(path);
  }
}

// -M: the list doubles as the index input when no index option was given; the matrix itself is timed
// as a query of its own (both "lasted" rows are printed again, as the reference does)
void run_matrix(nqhost::Index &ix, const Parsed &o, RunClock &clk) {
  if (!o.has(MATRIX)) return;
  const string list = o.last(MATRIX);
  warn_if_unreadable(list);
  if (!o.has(LIST) && !o.has(LISTLINES)) {
    clk.run_begin = system_clock::now();
    {
      ListDir here(list);
      ix.insert_file_of_file_whole(leaf_of(list));
    }
    clk.index_done();
  }
  ListDir here(list);
  clk.run_begin = system_clock::now();
  ix.query_matrix();
  RunClock::row("| Query lasted (s)                  |", clk.run_begin, system_clock::now());
}

int int_opt(const Parsed &o, Opt id, int dflt) { return o.has(id) ? atoi(o.last(id).c_str()) : dflt; }

// Which options need which optional calls of the engine (nqhost::Index::lacks), in the order a run is refused for
// them: a row per Feature, in its order.
using Feature = nqhost::Index::Feature;
const struct { Opt asked_by[3]; Feature feature; } kNeeds[] = {
    {{MERGE, MERGE, MERGE}, Feature::APPEND},
    {{NOVEL, NOVEL, NOVEL}, Feature::DEREPLICATION_FROM},
    {{NOVEL, REMOVE, DEREP_DUMP}, Feature::RETAIN},
    {{PAN, PAN, PAN}, Feature::UNITE},
    {{NEIGHBORS, CLUSTER, CLUSTER}, Feature::SELF_JOIN},
    {{DEREP, DEREP_DUMP, DEREP_DUMP}, Feature::DEREPLICATION},
    {{MST, LINKAGE, TREE}, Feature::LINKAGE},
    {{AUDIT, AUDIT, AUDIT}, Feature::AUDIT},
    {{LCA, LCA, LCA}, Feature::LCA},
    {{COVER, COVER, COVER}, Feature::COVER},
    {{SIZES, CONTAINMENT, CONTAINMENT}, Feature::SIZES},
    {{MIN_CONTAINMENT, MIN_CONTAINMENT, MIN_CONTAINMENT}, Feature::CONTAINED},
    {{COLLAPSE, COLLAPSE, COLLAPSE}, Feature::COLLAPSE},
    {{REPORT, REPORT, REPORT}, Feature::TALLY},
};
// the text of the first row in [first, last] that the options ask for and the engine lacks, else null (main has
// refusals of its own between the rows: the loop runs over one stretch of them at a time)
const char *engine_lacks(const Parsed &o, Feature first, Feature last) {
  for (size_t r = (size_t)first; r <= (size_t)last; ++r)
    for (Opt opt : kNeeds[r].asked_by)
      if (const char *text = o.has(opt) ? nqhost::Index::lacks(kNeeds[r].feature) : nullptr) return text;
  return nullptr;
}

}  // namespace

int main(int argc, char *argv[]) {
  if (argc > 0) { --argc; ++argv; }
  const Parsed o = parse(argc, argv);
  if (o.error) {
    cout << "Bad usage!!!" << endl;
    return EXIT_FAILURE;
  }
  if (o.has(HELP) || argc == 0) {
    print_usage();
    return EXIT_SUCCESS;
  }
  for (size_t i = 0; i < o.non_options.size(); ++i)
    cout << "Non-option argument #" << i << " is " << o.non_options[i] << endl
         << "Ignoring unknown argument '" << o.non_options[i] << "'" << endl;
  if (!o.non_options.empty()) {
    cout << "Bad usage!!!" << endl;
    return EXIT_FAILURE;
  }
  const int K = int_opt(o, KMER, 31), S = int_opt(o, FETCH, 15), H = int_opt(o, HHL, 4), W = int_opt(o, WORD, 12);
  const double min_jaccard = o.has(MIN) ? atof(o.last(MIN).c_str()) : 0;
  const int device = int_opt(o, DEVICE, -1), n_gpus = int_opt(o, GPUS, 1), resident_mib = int_opt(o, RESIDENT, 0);
  const string out_file = o.has(OUTPUT) ? o.last(OUTPUT) : "niqkiOutput.gz";
  // --top: the first k lines of each query's list (count descending, the larger gid first among equal counts)
  uint32_t top_k = 0;
  if (o.has(TOP)) {
    const long long v = strtoll(o.last(TOP).c_str(), nullptr, 10);
    if (v < 0 || v > (long long)UINT32_MAX) {
      fprintf(stderr, "Option 'top' requires a number in 0..%u\n", UINT32_MAX);
      cout << "Bad usage!!!" << endl;
      return EXIT_FAILURE;
    }
    top_k = (uint32_t)v;
  }

  const auto refused = [](const char *text) {
    cerr << "niqki: " << text << endl;
    return EXIT_FAILURE;
  };
  // the self-join asks one index about itself: a slot shard of a --gpus group sees partial counts; and only a
  // single-GPU index can drop genomes or take the genomes of a dump
  const bool linkage = o.has(MST) || o.has(LINKAGE) || o.has(TREE);
  if (n_gpus > 1 && (o.has(NEIGHBORS) || o.has(CLUSTER) || o.has(DEREP) || o.has(REMOVE) || o.has(DEREP_DUMP) || o.has(MERGE) || o.has(NOVEL) || linkage || o.has(AUDIT)))
    return refused("the self-join (--neighbors, --cluster, --derep), dropping genomes and merging dumps (--merge, --novel) need a single-GPU index (--gpus 1)");
  // the union is taken over the whole sketches of one device's store
  if (n_gpus > 1 && o.has(PAN)) return refused("--pan needs a single-GPU index (--gpus 1)");
  if (const char *text = engine_lacks(o, Feature::APPEND, Feature::LINKAGE)) return refused(text);
  // the two shares belong to the entries of the plain list, and the registers are read from whole sketches on one device
  if (o.has(CONTAINMENT)) {
    if (o.has(COVER) || o.has(COLLAPSE) || o.has(LCA))
      return refused("--containment extends the plain hit list: --cover, --collapse and --lca replace it, choose one");
    if (n_gpus > 1) return refused("--containment needs a single-GPU index (--gpus 1)");
  }
  if (n_gpus > 1 && o.has(SIZES)) return refused("--sizes needs a single-GPU index (--gpus 1)");
  if (const char *text = engine_lacks(o, Feature::SIZES, Feature::SIZES)) return refused(text);
  // --min-containment: 0 < x <= 1 as a share of 2^32, rounded up (1 is NIQKI_CONTAIN_ONE); --containment-of: whose share
  uint32_t min_share = 0, contain_mode = NIQKI_CONTAIN_QUERY;
  if (o.has(MIN_CONTAINMENT)) {
    const string &a = o.last(MIN_CONTAINMENT);
    char *end = nullptr;
    errno = 0;
    const double x = strtod(a.c_str(), &end);
    if (a.empty() || a[0] == ' ' || end == a.c_str() || *end != 0 || errno || !(x > 0.0) || !(x <= 1.0)) {
      fprintf(stderr, "Option 'min-containment' requires a number x with 0 < x <= 1\n");
      cout << "Bad usage!!!" << endl;
      return EXIT_FAILURE;
    }
    const double scaled = std::ceil(x * 4294967296.0);   // (exact: a power of two times a double)
    min_share = scaled >= 4294967295.0 ? NIQKI_CONTAIN_ONE : (uint32_t)scaled;
  }
  if (o.has(CONTAINMENT_OF)) {
    if (!o.has(MIN_CONTAINMENT)) return refused("--containment-of needs --min-containment");
    const string &a = o.last(CONTAINMENT_OF);
    if (a == "query") contain_mode = NIQKI_CONTAIN_QUERY;
    else if (a == "genome") contain_mode = NIQKI_CONTAIN_GENOME;
    else if (a == "either") contain_mode = NIQKI_CONTAIN_MAX;
    else {
      fprintf(stderr, "Option 'containment-of' requires query, genome or either\n");
      cout << "Bad usage!!!" << endl;
      return EXIT_FAILURE;
    }
  }
  // the shares select from the plain list, on one device from whole counts and the registers of whole sketches
  if (o.has(MIN_CONTAINMENT)) {
    if (o.has(COVER) || o.has(COLLAPSE) || o.has(LCA))
      return refused("--min-containment selects from the plain hit list: --cover, --collapse and --lca replace it, choose one");
    if (n_gpus > 1) return refused("--min-containment needs a single-GPU index (--gpus 1)");
    if (const char *text = engine_lacks(o, Feature::CONTAINED, Feature::CONTAINED)) return refused(text);
    if (const char *text = nqhost::Index::lacks(Feature::SIZES)) return refused(text);   // (the sizes come from the registers)
  }

  // --audit-k: how many of a genome's nearest neighbours vote, a plain integer
  uint32_t audit_k = 1;
  if (o.has(AUDIT_K)) {
    const string &a = o.last(AUDIT_K);
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(a.c_str(), &end, 10);
    if (a.empty() || a[0] == '+' || a[0] == ' ' || end == a.c_str() || *end != 0 || errno || v < 1 || v > 63) {
      fprintf(stderr, "Option 'audit-k' requires an integer in 1..63\n");
      cout << "Bad usage!!!" << endl;
      return EXIT_FAILURE;
    }
    audit_k = (uint32_t)v;
  }
  // the audit checks the label file the run acts on
  if (o.has(AUDIT)) {
    if (!o.has(COLLAPSE) && !o.has(PAN)) return refused("--audit needs --collapse or --pan");
    if (const char *text = engine_lacks(o, Feature::AUDIT, Feature::AUDIT)) return refused(text);
  }

  // --lca-top: thousandths of the best count, a plain integer
  uint32_t lca_permille = 100;
  if (o.has(LCA_TOP)) {
    const string &a = o.last(LCA_TOP);
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(a.c_str(), &end, 10);
    if (a.empty() || a[0] == '+' || a[0] == ' ' || end == a.c_str() || *end != 0 || errno || v < 0 || v > 1000) {
      fprintf(stderr, "Option 'lca-top' requires an integer in 0..1000\n");
      cout << "Bad usage!!!" << endl;
      return EXIT_FAILURE;
    }
    lca_permille = (uint32_t)v;
  }
  // the report tallies the rows of the LCA query
  if (o.has(REPORT) && !o.has(LCA)) return refused("--report needs --lca");
  // the taxon is folded on one device from whole counts
  if (o.has(LCA)) {
    if (n_gpus > 1) return refused("--lca needs a single-GPU index (--gpus 1)");
    if (o.has(COVER)) return refused("--lca and --cover both replace a query's list: choose one");
    if (const char *text = engine_lacks(o, Feature::LCA, Feature::LCA)) return refused(text);
    if (const char *text = engine_lacks(o, Feature::TALLY, Feature::TALLY)) return refused(text);
  }
  if (o.has(COLLAPSE) && o.has(COVER)) return refused("--collapse and --cover both replace a query's list: choose one");
  // the cover reads whole counts and the winner's column of a device-resident sketch store
  if (o.has(COVER)) {
    if (n_gpus > 1) return refused("--cover needs a single-GPU index (--gpus 1)");
    if (resident_mib > 0) return refused("--cover needs a resident index (--resident-mib 0): a paged index keeps its sketch store in host memory");
    if (const char *text = engine_lacks(o, Feature::COVER, Feature::COVER)) return refused(text);
  }
  // the collapsed list is selected on one device from whole counts
  if (o.has(COLLAPSE) && !o.has(LCA)) {   // (beside --lca the file supplies the labels only: no collapsed query runs)
    if (n_gpus > 1) return refused("--collapse needs a single-GPU index (--gpus 1)");
    if (const char *text = engine_lacks(o, Feature::COLLAPSE, Feature::COLLAPSE)) return refused(text);
  }

  const char *rule = "+-----------------------------------+-------------------------------+";
  cout << "+-------------------------------------------------------------------+" << endl
       << "|                            Informations                           |" << endl
       << rule << endl;
  std::unique_ptr<nqhost::Index> ix;
  try {
    if (o.has(LOAD)) ix.reset(new nqhost::Index(o.last(LOAD), true, out_file, device, n_gpus, resident_mib, top_k));
    else ix.reset(new nqhost::Index(S, K, W, H, out_file, min_jaccard, device, n_gpus, resident_mib, top_k));
    ix->cover = o.has(COVER);
    ix->containment = o.has(CONTAINMENT);
    ix->min_share = min_share;
    ix->contain_mode = contain_mode;
    if (o.has(REPORT)) ix->report = o.last(REPORT);
    if (const unsigned expect = (unsigned)int_opt(o, GENOME_SIZE, 0)) ix->select_best_H(expect);   // src/niqki.cpp:303-305

    const uint32_t n_loaded = (uint32_t)ix->getNbGenomes();   // --novel: the genomes of -L are given (none without -L)
    RunClock clk;
    for (const Phase &ph : kIndexPhases) run_phase(*ix, o, ph);
    if (o.has(DOWNLAD)) cout << "--indexdownload needs network access and is not part of this build" << endl;
    if (o.has(MERGE))   // the one option of which every occurrence counts
      for (const string &dump : o.opts.at(MERGE)) ix->merge_dump(dump);
    RunClock::tp novel_begin, novel_end, remove_begin, remove_end, pan_begin, pan_end, audit_begin, audit_end;
    vector<uint64_t> audit_totals;
    // the row of the audit phase and the genomes per verdict
    const auto audit_done = [&]() {
      RunClock::row("| Audit lasted (s)                  |", audit_begin, audit_end);
      cout << "Audit:";
      for (size_t v = 0; v < audit_totals.size(); ++v) cout << (v ? ", " : " ") << audit_totals[v] << " " << nqhost::Index::kAuditVerdicts[v];
      cout << endl;
    };
    if (o.has(NOVEL)) {
      novel_begin = system_clock::now();
      // the -J of THIS run where it is given: an index that -L loaded carries the min_score of its dump
      ix->keep_novel(n_loaded, o.has(MIN) ? niqki_min_score(min_jaccard, ix->lF) : ix->min_score, o.last(NOVEL));
      novel_end = system_clock::now();
    }
    if (o.has(REMOVE)) {   // after everything that indexes, before the dump: -L old --remove names -D new
      remove_begin = system_clock::now();
      ix->remove_listed(o.last(REMOVE));
      remove_end = system_clock::now();
    }
    if (o.has(PAN)) {   // ... and after the genomes that leave: -L db.dump --pan species.tsv -D species.dump
      if (o.has(AUDIT)) {   // the file is checked before it is acted on: the union cannot be undone
        audit_begin = system_clock::now();
        audit_totals = ix->audit_to_file(o.last(AUDIT), audit_k, o.last(PAN), "--pan");
        audit_end = system_clock::now();
      }
      pan_begin = system_clock::now();
      ix->unite_listed(o.last(PAN));
      pan_end = system_clock::now();
    }
    if (o.has(DUMP)) ix->dump_index_disk(o.last(DUMP));
    clk.index_done();
    if (o.has(NOVEL)) RunClock::row("| Novelty filter lasted (s)         |", novel_begin, novel_end);
    if (o.has(REMOVE)) RunClock::row("| Remove lasted (s)                 |", remove_begin, remove_end);
    if (o.has(PAN) && o.has(AUDIT)) audit_done();
    if (o.has(PAN)) RunClock::row("| Pan sketches lasted (s)           |", pan_begin, pan_end);
    if (o.has(CLUSTER)) {   // a phase of its own between indexing and the queries
      ix->cluster_to_file(o.last(CLUSTER));
      const RunClock::tp now = system_clock::now();
      RunClock::row("| Cluster lasted (s)                |", clk.index_end, now);
      clk.index_end = now;
    }
    if (o.has(DEREP) || o.has(DEREP_DUMP)) {   // ... and so is the dereplication, after the clusters where both are asked for
      // one engine call for the list and the dump; after --derep-dump the index in memory is the dereplicated one
      ix->dereplicate(o.has(DEREP) ? o.last(DEREP) : string(), o.has(DEREP_DUMP) ? o.last(DEREP_DUMP) : string());
      const RunClock::tp now = system_clock::now();
      RunClock::row("| Dereplication lasted (s)          |", clk.index_end, now);
      clk.index_end = now;
    }
    if (linkage) {   // ... and the linkage phase: one engine call for the three files; after --derep-dump of the dereplicated index
      ix->linkage_to_files(o.has(MST) ? o.last(MST) : string(), o.has(LINKAGE) ? o.last(LINKAGE) : string(),
                           o.has(TREE) ? o.last(TREE) : string());
      const RunClock::tp now = system_clock::now();
      RunClock::row("| Linkage lasted (s)                |", clk.index_end, now);
      clk.index_end = now;
    }
    run_matrix(*ix, o, clk);
    // after everything that changes the index in memory (-M may index its list): the names are those of the final index
    if (o.has(AUDIT) && !o.has(PAN)) {   // a phase of its own, where the --collapse file is applied
      audit_begin = system_clock::now();
      audit_totals = ix->audit_to_file(o.last(AUDIT), audit_k, o.last(COLLAPSE), "--collapse");
      audit_end = system_clock::now();
      audit_done();
      clk.index_end += audit_end - audit_begin;   // (the query row does not count it)
    }
    if (o.has(SIZES)) {   // a phase of its own: the index is final, the names are those the queries will print
      const RunClock::tp sizes_begin = system_clock::now();
      ix->sizes_to_file(o.last(SIZES));
      const RunClock::tp sizes_end = system_clock::now();
      RunClock::row("| Sizes lasted (s)                  |", sizes_begin, sizes_end);
      clk.index_end += sizes_end - sizes_begin;   // (the query row does not count it)
    }
    if (o.has(LCA)) ix->set_lca(o.last(LCA), lca_permille, o.has(COLLAPSE) ? o.last(COLLAPSE) : string());
    else if (o.has(COLLAPSE)) ix->set_collapse(o.last(COLLAPSE));
    if (o.has(NEIGHBORS)) ix->query_neighbors();
    for (const Phase &ph : kQueryPhases) run_phase(*ix, o, ph);
    if (o.has(REPORT)) ix->write_report();
    if (o.has(MIN_CONTAINMENT)) cout << "Hits without a size estimate: " << ix->unsized_hits << endl;
    ix->outfile->close();
    const RunClock::tp done = system_clock::now();
    RunClock::row("| Query lasted (s)                  |", clk.index_end, done);
    RunClock::row("| Whole run lasted (s)              |", clk.run_begin, done);
  } catch (const std::exception &e) {
    cerr << "niqki: " << e.what() << endl;
    return EXIT_FAILURE;
  }

  if (o.has(LOGO)) {
    ifstream art("../resources/niqki.ascii");
    if (!art.is_open()) cout << "Unable to open file :'../resources/niqki.ascii'" << endl;
    for (string line; art.is_open() && getline(art, line);) cout << line << '\n';
    return EXIT_SUCCESS;
  }
  cout << rule << endl;
  box_row("| k-mer size                        |", K);
  box_row("| S                                 |", S);
  box_row("| Number of fingerprints            |", ix->F);
  box_row("| W                                 |", W);
  box_row("| H                                 |", H);
  box_row("| Number of indexed genomes         |", ix->getNbGenomes());
  cout << rule << endl;
  return EXIT_SUCCESS;
}
