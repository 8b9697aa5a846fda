// nq_group.h -- internal: the state of a slot-sharded group (niqki_group_*, include/niqki_hip.h) and the seam
// between its two halves.  nq_group.hip is the exchange PROTOCOL (slices, gather, look-up, sum, hits, dense
// redo) and the C ABI; nq_group_transport.hip is HOW bytes cross ranks (rccl / local / ipc).  The protocol
// reaches the transport only through the functions of namespace nqg below.
#pragma once
#include "nq_handle.h"

#include <array>
#include <string>
#include <vector>

constexpr uint32_t kMaxWorld = 64;

// The exchange buffers: what a rank WRITES for its peers to read (ipc: the four views of one exported arena).
enum Xbuf : uint32_t { kSend, kCand, kMine, kCounts, kXbufs };   // slices, candidate blob, my partial counts, counter rows

struct niqki_group_transport;   // communicators / ipc state (nq_group_transport.hip)

struct niqki_group {
  uint32_t world = 1, n_local = 1, first = 0;
  std::vector<niqki_index *> sh;     // local shards, rank first + l
  enum Transport { kLocal, kRccl, kIpc } transport = kLocal;
  niqki_group_transport *tp = nullptr;
  int exchange = 0;                  // 0 = choose, 1 = sparse, 2 = dense reduce-scatter
  uint32_t cand_cap = 256;
  uint32_t surv_cap = 1024;          // survivors (partial count >= half the candidate threshold) kept per query and shard
  uint64_t overflows = 0;            // sparse steps redone densely
  bool wide = false;                 // S = 16: cross-shard sums reach 2^16, they travel and add up as u32
  std::string err;
  struct Ws {
    nqi::Buf xbuf[kXbufs];
    nqi::Buf recv, allsk, cand_all, tot, red, flag, hitoff, hc, hg, stpad, surv, keys, nhit, rows16, sum32;
    hipEvent_t ev = nullptr;
    // every buffer of the workspace (a new one joins here)
    std::array<nqi::Buf *, kXbufs + 15> all() {
      return {&xbuf[kSend], &xbuf[kCand], &xbuf[kMine], &xbuf[kCounts], &recv, &allsk, &cand_all, &tot, &red, &flag,
              &hitoff, &hc, &hg, &stpad, &surv, &keys, &nhit, &rows16, &sum32};
    }
  };
  std::vector<Ws> ws;
  // a query batch between niqki_group_query_begin and _end
  struct Pending {
    bool active = false, sparse = false, host = false;
    uint32_t per = 0, N = 0;
    uint64_t capacity = 0;
    uint64_t *const *hit_off = nullptr;
    uint32_t *const *hit_counts = nullptr, *const *hit_gids = nullptr;
    std::vector<uint64_t *> off_v;
    std::vector<uint32_t *> hc_v, hg_v;
  } pend;
  uint32_t *host_flags = nullptr;    // pinned: {candidate overflow, ipc wait timeout} of the batch in flight
  hipEvent_t ev_flags = nullptr;
};

inline int gfail(niqki_group *g, int code, const std::string &msg) {
  if (g) g->err = msg;
  return code;
}

#define NQ_G(g, l, call)                                                                      \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_) return gfail(g, rc_, std::string(#call) + ": " + niqki_last_error((g)->sh[l]));  \
  } while (0)
#define NQ_GH(g, call)                                                                        \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) return gfail(g, NIQKI_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ---- the transport, as the protocol sees it --------------------------------------------------------
namespace nqg {

using RecvBuf = nqi::Buf niqki_group::Ws::*;   // where a collective leaves its result, per local rank

// Chooses the transport (NIQKI_GROUP_TRANSPORT, who shares a device) and sets it up: communicators (rccl), the
// processes' shared block and sequence words (ipc).  The shards are validated, g->ws sized.  On failure g->err says why.
int open(niqki_group *g, const uint8_t *id, bool shared_device);
// Undoes open() and whatever reserve() made; the streams have drained.  ipc: the xbuf views of ws[0] are cleared.
void close(niqki_group *g);
// The group id of niqki_group_new_id (an ncclUniqueId, or random bytes for ipc).
int new_id(uint8_t *id);
// ipc: the exchange buffers of the coming batch hold at least need[b] bytes, made and mapped by all ranks BEFORE any
// of them is used.  A no-op on the other transports, whose buffers are plain scratch (nqi::ensure).
int reserve(niqki_group *g, const size_t need[kXbufs]);
// Before this rank overwrites exchange buffer b: its previous contents have been read by everybody.
// (A no-op but on ipc: the other transports' collectives are ordered by their own streams / RCCL.)
int before_write(niqki_group *g, Xbuf b);
// recv[l] = [world][bytes] <- send[s] + rank(l) * bytes of every rank s (bytes: a multiple of 16)
int all_to_all(niqki_group *g, Xbuf send, RecvBuf recv, size_t bytes);
// recv[l] = [world][bytes] <- send[s] of every rank s (bytes: a multiple of 16)
int all_gather(niqki_group *g, Xbuf send, RecvBuf recv, size_t bytes);
// recv[l][i] = sum over ranks s of send[s][rank(l) * count + i], u32 words
int reduce_scatter_u32(niqki_group *g, Xbuf send, RecvBuf recv, size_t count);
// How many ranks the transport itself knows of: the communicator's size as RCCL reports it, the peers whose
// sequence words this process has mapped (ipc), the shards of the process (local).
int ranks_seen(const niqki_group *g, uint64_t *n);
// ipc: the device word a wait kernel sets when a peer did not answer in time; null on the other transports.
const uint32_t *timeout_flag(const niqki_group *g);
uint64_t ipc_words_kind(const niqki_group *g);   // 0 coarse, 1 fine-grained, 2 host block
uint64_t ipc_arena_fine(const niqki_group *g);

}  // namespace nqg
