// nq_group_transport.hip -- how the bytes of a slot-sharded group's exchange cross ranks: the functions of
// namespace nqg (nq_group.h), which is all the protocol in nq_group.hip knows of a transport.  No protocol step
// lives here: three collectives over the exchange buffers, their set-up and their ordering.
//
//   rccl   librccl, loaded on first use -- one communicator per local rank, so the same code serves one
//          rank per process (bench.py under torch.distributed.run) and all ranks in one process
//          (`niqki --gpus N`).
//   local  all ranks in one process and two shards share a device (tests, emulation of G shards on one
//          GPU), which RCCL refuses: plain device-to-device copies and a summing kernel stand in for
//          the collectives.
//   ipc    NIQKI_GROUP_TRANSPORT=ipc, one rank per process: every rank maps its peers' exchange buffers
//          (hipIpcGetMemHandle / hipIpcOpenMemHandle, handles passed through a POSIX shared-memory block
//          named by the group id) and PULLS what it needs with a copy or summing kernel -- over xGMI
//          that is a direct all-to-all on all links instead of a ring.  Ordering is by sequence numbers in
//          device memory: tiny signal / wait kernels on the ranks' streams, no host synchronisation in a
//          step.  Ranks may share a device (how the N > 1 path runs on a one-GPU box).
#include "nq_group.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {

using nqi::Buf;

// ---- librccl, resolved at first use ---------------------------------------------------------
struct Rccl {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclReduceScatter) ReduceScatter = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string why;
  bool load() {
    if (lib) return true;
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) { why = std::string("cannot load librccl: ") + dlerror(); return false; }
#define NQ_SYM(field, sym)                                                  \
  field = (decltype(field))dlsym(lib, sym);                                 \
  if (!field) { why = std::string("librccl lacks ") + sym; lib = nullptr; return false; }
    NQ_SYM(GetUniqueId, "ncclGetUniqueId")
    NQ_SYM(CommInitRank, "ncclCommInitRank")
    NQ_SYM(CommDestroy, "ncclCommDestroy")
    NQ_SYM(CommCount, "ncclCommCount")
    NQ_SYM(GroupStart, "ncclGroupStart")
    NQ_SYM(GroupEnd, "ncclGroupEnd")
    NQ_SYM(Send, "ncclSend")
    NQ_SYM(Recv, "ncclRecv")
    NQ_SYM(AllGather, "ncclAllGather")
    NQ_SYM(ReduceScatter, "ncclReduceScatter")
    NQ_SYM(GetErrorString, "ncclGetErrorString")
#undef NQ_SYM
    return true;
  }
};
Rccl &rccl() {
  static Rccl r;
  return r;
}

// ---- ipc transport: the block the processes of a group share ------------------------------------
constexpr uint32_t kIpcBufs = kXbufs;   // exchange buffers a rank exposes: send (slices), cand, mine, counts
constexpr uint32_t kIpcMagic = 0x4E514950u;
struct IpcRank {
  // Handles name whole allocations (hipMalloc may carve a pointer out of a larger block, whose base is what
  // hipIpcGetMemHandle takes): the pointer is base + offset in the owner's and in every peer's mapping.
  hipIpcMemHandle_t flags;            // the rank's sequence words (below)
  uint64_t flags_off;
  hipIpcMemHandle_t arena;            // ONE allocation holds the rank's exchange buffers
  uint64_t arena_off;
  uint64_t buf_off[kIpcBufs];         // ... buffer i at arena + buf_off[i]
  uint64_t gen;                       // bumped when `arena` names a new allocation
  int32_t device;
  uint32_t words_kind;                // where the rank's sequence words live (kWords*)
  uint32_t arena_fine;                // 1 = the arena is fine-grained device memory
  char pci[32];                       // the rank's device (hipDeviceGetPCIBusId): peers check that they can reach it
};
// Memory kinds of a rank's sequence words.  A peer GPU polls them from a RUNNING kernel, so they must be
// coherent at system scope by contract, not by observed behaviour: fine-grained device memory (what RCCL keeps
// its own flags in), or -- where that cannot be made or exported -- words in the POSIX shared block itself,
// page-locked and mapped into every process (hipHostRegister: host-coherent).  Plain hipMalloc memory
// (coarse-grained: coherent across devices only at kernel boundaries) is the last resort and is reported.
constexpr uint32_t kWordsCoarse = 0, kWordsFine = 1, kWordsHost = 2;
constexpr uint32_t kFlagWordsMax = 64;
struct IpcShared {
  std::atomic<uint32_t> init, bar_count, bar_gen, abort;
  std::atomic<uint32_t> export_lock;   // one rank at a time allocates and exports its arena
  IpcRank r[kMaxWorld];
  alignas(256) uint32_t host_words[kMaxWorld][kFlagWordsMax];   // kWordsHost: rank r's sequence words
};
// sequence words of a rank (device memory, mapped by every peer): ready[b] = uses of buffer b whose data
// is complete, done[b] = uses whose data this rank has finished reading from ALL peers, err = a wait timed out
constexpr uint32_t kFlagReady = 0, kFlagDone = kIpcBufs, kFlagErr = 2 * kIpcBufs, kFlagWords = kFlagWordsMax;

}  // namespace

namespace nq {

// ---- ipc transport kernels ------------------------------------------------------------------------
struct FlagPtrs { uint32_t *p[kMaxWorld]; };
struct PeerSrc { const uint8_t *p[kMaxWorld]; };

// everything enqueued before on this stream is complete and visible: publish sequence number `seq`
__global__ void ipc_signal_kernel(uint32_t *word, uint32_t seq) {
  __threadfence_system();
  __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// lane r waits until rank r's word has reached seq (one wave; every lane leaves after `timeout` ticks
// of the 100 MHz clock at the latest and reports through *err)
__global__ __launch_bounds__(64) void ipc_wait_kernel(FlagPtrs f, uint32_t world, uint32_t word, uint32_t seq, uint32_t *err,
                                                     unsigned long long timeout) {
  const uint32_t r = threadIdx.x;
  if (r >= world) return;
  const unsigned long long t0 = wall_clock64();
  while ((int32_t)(__hip_atomic_load(f.p[r] + word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {
    if (wall_clock64() - t0 > timeout) {
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
    __builtin_amdgcn_s_sleep(32);
  }
}
// dst[s * bytes ..] = src.p[s][off ..  off + bytes) for every rank s (bytes and off multiples of 16)
__global__ __launch_bounds__(256) void ipc_pull_kernel(PeerSrc src, uint64_t off, uint64_t bytes, uint8_t *dst) {
  const uint32_t s = blockIdx.y;
  const uint4 *in = (const uint4 *)(src.p[s] + off);
  uint4 *out = (uint4 *)(dst + (uint64_t)s * bytes);
  const uint64_t n = bytes / 16, step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) out[i] = in[i];
}

struct SumSrc { const uint32_t *p[kMaxWorld]; };
// stand-in for reduce-scatter inside one process: out[i] = sum over ranks of src[r][off + i]
__global__ __launch_bounds__(256) void sum_rows_kernel(SumSrc src, uint32_t G, uint64_t off, uint64_t n, uint32_t *out) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    uint32_t s = 0;
    for (uint32_t r = 0; r < G; ++r) s += src.p[r][off + i];
    out[i] = s;
  }
}

}  // namespace nq

struct niqki_group_transport {
  std::vector<ncclComm_t> comm;      // per local rank (kRccl)
  // ipc transport (n_local == 1)
  struct Ipc {
    IpcShared *shm = nullptr;
    std::string name;
    uint32_t *flags = nullptr;                 // my sequence words (device)
    uint32_t *peer_flags[kMaxWorld] = {};      // every rank's, mine included
    void *peer_buf[kMaxWorld][kIpcBufs] = {};  // mapped exchange buffers (mine: the local pointer)
    void *peer_base[kMaxWorld] = {};           // what hipIpcOpenMemHandle returned for a peer's arena / flags
    void *peer_flags_base[kMaxWorld] = {};
    uint64_t peer_gen[kMaxWorld] = {};
    Buf arena;                                 // my exchange buffers (ws.xbuf[] are views of it)
    bool ready = false;                        // ipc_setup went through: peers exist and wait in barriers
    uint32_t words_kind = kWordsCoarse;        // where MY sequence words live
    bool arena_fine = false;                   // my arena is fine-grained device memory
    bool shm_registered = false;               // the shared block is page-locked and mapped for this device
    uint32_t (*host_words_dev)[kFlagWordsMax] = nullptr;   // device view of IpcShared::host_words
    uint32_t seq[kIpcBufs] = {};               // uses of each exchange buffer so far
  } ipc;
};

namespace {

#define NQ_GN(g, call)                                                                        \
  do {                                                                                        \
    ncclResult_t r_ = (call);                                                                 \
    if (r_ != ncclSuccess) return gfail(g, NIQKI_E_HIP, std::string(#call) + ": " + rccl().GetErrorString(r_)); \
  } while (0)

// An RCCL group call that is closed on EVERY way out: a ncclSend / ncclRecv / collective that fails between
// GroupStart and GroupEnd must not leave the communicators with an open group (the NQ_G* macros return from inside).
struct RcclGroupScope {
  bool open = false;
  ncclResult_t begin() {
    const ncclResult_t r = rccl().GroupStart();
    open = r == ncclSuccess;
    return r;
  }
  ncclResult_t end() {
    open = false;
    return rccl().GroupEnd();
  }
  ~RcclGroupScope() {
    if (open) (void)rccl().GroupEnd();
  }
};

// ---- ipc transport, host side ---------------------------------------------------------------------
double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
constexpr double kIpcHostTimeout = 120.0;                       // seconds a process waits for its peers
constexpr unsigned long long kIpcDeviceTimeout = 3000000000ull; // 30 s of the 100 MHz clock for a wait kernel

// all processes of the group have arrived (sense-reversing counter in the shared block)
int ipc_barrier(niqki_group *g) {
  IpcShared *sh = g->tp->ipc.shm;
  const uint32_t gen = sh->bar_gen.load(std::memory_order_acquire);
  if (sh->bar_count.fetch_add(1, std::memory_order_acq_rel) + 1 == g->world) {
    sh->bar_count.store(0, std::memory_order_relaxed);
    sh->bar_gen.fetch_add(1, std::memory_order_release);
    return NIQKI_OK;
  }
  const double t0 = now_s();
  while (sh->bar_gen.load(std::memory_order_acquire) == gen) {
    if (sh->abort.load(std::memory_order_relaxed)) return gfail(g, NIQKI_E_STATE, "a peer process of the group gave up");
    if (now_s() - t0 > kIpcHostTimeout) {
      sh->abort.store(1, std::memory_order_relaxed);
      return gfail(g, NIQKI_E_STATE, "timed out waiting for the other processes of the group");
    }
    usleep(50);
  }
  return NIQKI_OK;
}

int ipc_export_alloc(niqki_group *g, size_t bytes, bool fine, void **out, hipIpcMemHandle_t *h, uint64_t *off);
bool env_is(const char *name, const char *value) {
  const char *e = std::getenv(name);
  return e && !std::strcmp(e, value);
}
// the shared block page-locked and mapped for my device (kWordsHost words of any rank are read through it)
int ipc_register_block(niqki_group *g) {
  auto &ic = g->tp->ipc;
  if (ic.shm_registered) return NIQKI_OK;
  NQ_GH(g, hipSetDevice(g->sh[0]->device));
  NQ_GH(g, hipHostRegister(ic.shm, sizeof(IpcShared), hipHostRegisterMapped | hipHostRegisterPortable));
  void *d = nullptr;
  hipError_t e = hipHostGetDevicePointer(&d, ic.shm->host_words, 0);
  if (e != hipSuccess) { (void)hipHostUnregister(ic.shm); return gfail(g, NIQKI_E_HIP, std::string("hipHostGetDevicePointer(shared block): ") + hipGetErrorString(e)); }
  ic.host_words_dev = (uint32_t (*)[kFlagWordsMax])d;
  ic.shm_registered = true;
  return NIQKI_OK;
}
// a peer's exported allocation into this process (a few tries: the same transient failure as on the export side)
hipError_t ipc_open(void **q, const hipIpcMemHandle_t &h) {
  hipError_t e = hipSuccess;
  for (int attempt = 0; attempt < 4; ++attempt) {
    if (attempt) { (void)hipGetLastError(); usleep(2000u << attempt); }
    e = hipIpcOpenMemHandle(q, h, hipIpcMemLazyEnablePeerAccess);
    if (e == hipSuccess) break;
  }
  return e;
}

int ipc_setup(niqki_group *g, const uint8_t *id) {
  auto &ic = g->tp->ipc;
  niqki_index *ix = g->sh[0];
  char name[64];
  std::snprintf(name, sizeof name, "/niqki_grp_%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x", id[0], id[1], id[2], id[3], id[4],
                id[5], id[6], id[7], id[8], id[9], id[10], id[11]);
  ic.name = name;
  int fd = -1;
  const double t0 = now_s();
  if (g->first == 0) {
    fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) return gfail(g, NIQKI_E_STATE, std::string("shm_open(create) failed for ") + name);
    if (ftruncate(fd, (off_t)sizeof(IpcShared)) != 0) { close(fd); shm_unlink(name); return gfail(g, NIQKI_E_STATE, "ftruncate of the group block failed"); }
  } else {
    for (;;) {
      fd = shm_open(name, O_RDWR, 0600);
      struct stat st;
      if (fd >= 0 && fstat(fd, &st) == 0 && (size_t)st.st_size >= sizeof(IpcShared)) break;
      if (fd >= 0) { close(fd); fd = -1; }
      if (now_s() - t0 > kIpcHostTimeout) return gfail(g, NIQKI_E_STATE, "rank 0 of the group never created its shared block");
      usleep(200);
    }
  }
  void *m = mmap(nullptr, sizeof(IpcShared), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (m == MAP_FAILED) return gfail(g, NIQKI_E_STATE, "mmap of the group block failed");
  ic.shm = (IpcShared *)m;
  if (g->first == 0) ic.shm->init.store(kIpcMagic, std::memory_order_release);
  else
    while (ic.shm->init.load(std::memory_order_acquire) != kIpcMagic) {
      if (now_s() - t0 > kIpcHostTimeout) return gfail(g, NIQKI_E_STATE, "the group's shared block was never initialised");
      usleep(50);
    }
  // my sequence words: fine-grained device memory that peers map (NIQKI_IPC_WORDS=host / coarse force the other kinds)
  NQ_GH(g, hipSetDevice(ix->device));
  IpcRank &me = ic.shm->r[g->first];
  auto give_up = [&](int code, const std::string &why) {   // the peers sit in a barrier: let them leave at once
    ic.shm->abort.store(1, std::memory_order_relaxed);
    return gfail(g, code, why);
  };
  int rc = NIQKI_OK;
  ic.words_kind = env_is("NIQKI_IPC_WORDS", "host") ? kWordsHost : env_is("NIQKI_IPC_WORDS", "coarse") ? kWordsCoarse : kWordsFine;
  if (ic.words_kind != kWordsHost) {
    void *fl = nullptr;
    rc = ipc_export_alloc(g, kFlagWords * 4, ic.words_kind == kWordsFine, &fl, &me.flags, &me.flags_off);
    if (rc && ic.words_kind == kWordsFine) { ic.words_kind = kWordsHost; rc = NIQKI_OK; }   // cannot be made or exported here
    else if (rc) return give_up(rc, g->err);
    else ic.flags = (uint32_t *)fl;
  }
  if (ic.words_kind == kWordsHost) {
    if ((rc = ipc_register_block(g))) return give_up(rc, g->err);
    ic.flags = ic.host_words_dev[g->first];
    std::memset(ic.shm->host_words[g->first], 0, sizeof ic.shm->host_words[g->first]);
  } else {
    NQ_GH(g, hipMemset(ic.flags, 0, kFlagWords * 4));
    NQ_GH(g, hipDeviceSynchronize());
  }
  me.words_kind = ic.words_kind;
  me.device = ix->device;
  std::memset(me.pci, 0, sizeof me.pci);
  if (hipDeviceGetPCIBusId(me.pci, (int)sizeof me.pci - 1, ix->device) != hipSuccess) { (void)hipGetLastError(); me.pci[0] = 0; }
  if ((rc = ipc_barrier(g))) return rc;
  for (uint32_t s = 0; s < g->world; ++s) {
    if (s == g->first) { ic.peer_flags[s] = ic.flags; continue; }
    const IpcRank &pr = ic.shm->r[s];
    // a peer on another device must be reachable from mine (xGMI / PCIe peer access): say so now rather than
    // through a wait kernel's 30 s time-out.  (A peer whose device this process cannot see is left to the mapping.)
    if (pr.pci[0] && me.pci[0] && std::strcmp(pr.pci, me.pci) != 0) {
      int peer_dev = -1, can = 1;
      if (hipDeviceGetByPCIBusId(&peer_dev, pr.pci) == hipSuccess && peer_dev >= 0) {
        if (hipDeviceCanAccessPeer(&can, ix->device, peer_dev) != hipSuccess) { (void)hipGetLastError(); can = 1; }
      } else {
        (void)hipGetLastError();
      }
      if (!can)
        return give_up(NIQKI_E_STATE, "ipc transport: device " + std::string(me.pci) + " (rank " + std::to_string(g->first) +
                                          ") has no peer access to device " + pr.pci + " (rank " + std::to_string(s) +
                                          "): use the rccl transport (NIQKI_GROUP_TRANSPORT=rccl)");
    }
    if (pr.words_kind == kWordsHost) {
      if ((rc = ipc_register_block(g))) return give_up(rc, g->err);
      ic.peer_flags[s] = ic.host_words_dev[s];
      continue;
    }
    void *q = nullptr;
    const hipError_t e = ipc_open(&q, pr.flags);
    if (e != hipSuccess) return give_up(NIQKI_E_HIP, std::string("hipIpcOpenMemHandle(sequence words of rank ") + std::to_string(s) + "): " + hipGetErrorString(e));
    ic.peer_flags_base[s] = q;
    ic.peer_flags[s] = (uint32_t *)((char *)q + pr.flags_off);
  }
  if ((rc = ipc_barrier(g))) return rc;
  if (g->first == 0) shm_unlink(name);   // everybody has it mapped: the name can go
  ic.ready = true;
  return NIQKI_OK;
}

void ipc_teardown(niqki_group *g) {
  auto &ic = g->tp->ipc;
  if (!ic.shm) return;
  for (uint32_t s = 0; s < g->world; ++s) {
    if (s == g->first) continue;
    if (ic.peer_base[s]) (void)hipIpcCloseMemHandle(ic.peer_base[s]);
    if (ic.peer_flags_base[s]) (void)hipIpcCloseMemHandle(ic.peer_flags_base[s]);
  }
  if (ic.flags && ic.words_kind != kWordsHost) (void)hipFree(ic.flags);
  ic.flags = nullptr;
  if (ic.shm_registered) { (void)hipHostUnregister(ic.shm); ic.shm_registered = false; }
  if (ic.arena.p) (void)hipFree(ic.arena.p);
  for (uint32_t b = 0; b < kIpcBufs; ++b) g->ws[0].xbuf[b] = Buf();   // (views of the arena)
  if (g->first == 0) shm_unlink(ic.name.c_str());   // (no-op once setup has finished)
  munmap(ic.shm, sizeof(IpcShared));
  ic.shm = nullptr;
}

// Device memory of `bytes` that peers can map: *h names the allocation it lies in, *off its place there
// (hipMalloc may carve a pointer out of a larger block, whose base is what hipIpcGetMemHandle takes).
// Exporting a fresh allocation now and then fails with "invalid argument" when two processes of one GPU do it
// at the same moment (seen once in four runs of two ranks on one MI355X, on the rank that came second): the
// ranks take turns, and a failed export is tried again on a new allocation.
// fine: fine-grained device memory (hipExtMallocWithFlags), coherent at system scope while kernels run.
int ipc_export_alloc(niqki_group *g, size_t bytes, bool fine, void **out, hipIpcMemHandle_t *h, uint64_t *off) {
  auto &ic = g->tp->ipc;
  const double t0 = now_s();
  uint32_t unlocked = 0;
  while (!ic.shm->export_lock.compare_exchange_weak(unlocked, 1u, std::memory_order_acquire)) {
    unlocked = 0;
    if (now_s() - t0 > kIpcHostTimeout) return gfail(g, NIQKI_E_STATE, "a peer never released the group's export lock");
    usleep(50);
  }
  void *p = nullptr, *base = nullptr;
  size_t sz = 0;
  hipError_t e = hipSuccess;
  for (int attempt = 0; attempt < 6; ++attempt) {
    if (p) { (void)hipFree(p); p = nullptr; usleep(2000u << attempt); }
    e = fine ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) : hipMalloc(&p, bytes);
    if (e != hipSuccess) { p = nullptr; break; }
    e = hipMemGetAddressRange((hipDeviceptr_t *)&base, &sz, (hipDeviceptr_t)p);
    if (e != hipSuccess) break;
    e = hipIpcGetMemHandle(h, base);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
  }
  ic.shm->export_lock.store(0u, std::memory_order_release);
  if (e != hipSuccess) {
    char msg[256];
    (void)hipGetLastError();
    std::snprintf(msg, sizeof msg, "%s exchange memory for peers (%zu bytes at %p, allocation %p of %zu bytes): %s",
                  fine ? "fine-grained" : "device", bytes, p, base, sz, hipGetErrorString(e));
    if (p) (void)hipFree(p);
    return gfail(g, NIQKI_E_HIP, msg);
  }
  *out = p;
  *off = (uint64_t)((char *)p - (char *)base);
  return NIQKI_OK;
}

// The exchange buffers of this batch, sized BEFORE any of them is used: every rank takes the same
// decisions (same shapes), so either nobody reallocates -- the steady state, no host traffic at all --
// or everybody does: then all streams drain, the old mappings are closed, the new buffers made, their
// handles published and mapped.
int ipc_prepare(niqki_group *g, const size_t need[kIpcBufs]) {
  auto &ic = g->tp->ipc;
  auto &w = g->ws[0];
  niqki_index *ix = g->sh[0];
  bool grow = false;
  for (uint32_t b = 0; b < kIpcBufs; ++b) grow |= need[b] > w.xbuf[b].n;
  if (!grow) return NIQKI_OK;
  NQ_GH(g, hipSetDevice(ix->device));
  NQ_GH(g, hipStreamSynchronize(ix->stream));
  int rc = ipc_barrier(g);   // every rank's stream has drained: nobody reads anybody's buffers
  if (rc) return rc;
  for (uint32_t s = 0; s < g->world; ++s)
    if (s != g->first && ic.peer_base[s]) {
      NQ_GH(g, hipIpcCloseMemHandle(ic.peer_base[s]));
      ic.peer_base[s] = nullptr;
      for (uint32_t b = 0; b < kIpcBufs; ++b) ic.peer_buf[s][b] = nullptr;
    }
  if ((rc = ipc_barrier(g))) return rc;
  // one allocation for the four buffers, each with a quarter of headroom (fewer remaps while batches grow)
  IpcRank &me = ic.shm->r[g->first];
  size_t off[kIpcBufs], size[kIpcBufs], total = 0;
  for (uint32_t b = 0; b < kIpcBufs; ++b) {
    const size_t have = w.xbuf[b].n;
    size[b] = need[b] > have ? need[b] + need[b] / 4 : have;
    size[b] = (size[b] + 255) & ~(size_t)255;
    off[b] = total;
    total += size[b];
  }
  if (ic.arena.p) NQ_GH(g, hipFree(ic.arena.p));
  ic.arena = Buf();
  void *arena = nullptr;
  // fine-grained like the words (peers read it while my later kernels run); plain device memory where that fails
  const bool want_fine = !env_is("NIQKI_IPC_ARENA", "coarse");
  rc = want_fine ? ipc_export_alloc(g, std::max<size_t>(total, 256), true, &arena, &me.arena, &me.arena_off) : NIQKI_E_HIP;
  ic.arena_fine = rc == NIQKI_OK;
  if (rc && (rc = ipc_export_alloc(g, std::max<size_t>(total, 256), false, &arena, &me.arena, &me.arena_off))) {
    ic.shm->abort.store(1, std::memory_order_relaxed);
    return rc;
  }
  me.arena_fine = ic.arena_fine ? 1u : 0u;
  ic.arena.p = arena;
  ic.arena.n = std::max<size_t>(total, 256);
  for (uint32_t b = 0; b < kIpcBufs; ++b) {
    Buf &buf = w.xbuf[b];
    buf.p = size[b] ? (char *)ic.arena.p + off[b] : nullptr;
    buf.n = size[b];
    me.buf_off[b] = off[b];
    ic.peer_buf[g->first][b] = buf.p;
  }
  me.gen += 1;
  if ((rc = ipc_barrier(g))) return rc;
  for (uint32_t s = 0; s < g->world; ++s) {
    if (s == g->first) continue;
    const IpcRank &pr = ic.shm->r[s];
    void *q = nullptr;
    NQ_GH(g, ipc_open(&q, pr.arena));
    ic.peer_base[s] = q;
    ic.peer_gen[s] = pr.gen;
    for (uint32_t b = 0; b < kIpcBufs; ++b) ic.peer_buf[s][b] = (char *)q + pr.arena_off + pr.buf_off[b];
  }
  return ipc_barrier(g);
}

// on my stream: wait until word `word` of every rank has reached seq
int ipc_wait_all(niqki_group *g, uint32_t word, uint32_t seq) {
  auto &ic = g->tp->ipc;
  nq::FlagPtrs f{};
  for (uint32_t s = 0; s < g->world; ++s) f.p[s] = ic.peer_flags[s];
  hipLaunchKernelGGL(nq::ipc_wait_kernel, dim3(1), dim3(64), 0, g->sh[0]->stream, f, g->world, word, seq, ic.flags + kFlagErr,
                     kIpcDeviceTimeout);
  NQ_GH(g, hipGetLastError());
  return NIQKI_OK;
}
int ipc_signal(niqki_group *g, uint32_t word, uint32_t seq) {
  hipLaunchKernelGGL(nq::ipc_signal_kernel, dim3(1), dim3(1), 0, g->sh[0]->stream, g->tp->ipc.flags + word, seq);
  NQ_GH(g, hipGetLastError());
  return NIQKI_OK;
}

// every local stream waits for everything enqueued so far on all local streams (local transport)
int cross_wait(niqki_group *g) {
  for (uint32_t l = 0; l < g->n_local; ++l) {
    NQ_GH(g, hipSetDevice(g->sh[l]->device));
    NQ_GH(g, hipEventRecord(g->ws[l].ev, g->sh[l]->stream));
  }
  for (uint32_t l = 0; l < g->n_local; ++l) {
    NQ_GH(g, hipSetDevice(g->sh[l]->device));
    for (uint32_t s = 0; s < g->n_local; ++s)
      if (s != l) NQ_GH(g, hipStreamWaitEvent(g->sh[l]->stream, g->ws[s].ev, 0));
  }
  return NIQKI_OK;
}

// ipc form of the three collectives: publish my buffer, wait for everybody's, pull (copy or sum), say so
template <typename Pull>
int ipc_collective(niqki_group *g, Xbuf b, Pull &&pull) {
  auto &ic = g->tp->ipc;
  NQ_GH(g, hipSetDevice(g->sh[0]->device));
  const uint32_t seq = ++ic.seq[b];
  int rc = ipc_signal(g, kFlagReady + (uint32_t)b, seq);
  if (!rc) rc = ipc_wait_all(g, kFlagReady + (uint32_t)b, seq);
  if (rc) return rc;
  for (uint32_t s = 0; s < g->world; ++s)
    if (!ic.peer_buf[s][b]) return gfail(g, NIQKI_E_STATE, "a peer's exchange buffer is not mapped");
  if ((rc = pull())) return rc;
  return ipc_signal(g, kFlagDone + (uint32_t)b, seq);
}

// all_to_all (own_part: rank l takes part l of every rank's buffer) and all_gather (every rank's whole buffer):
// recv[l] = [world][bytes] <- send[s] + (own_part ? rank(l) * bytes : 0) of every rank s
int exchange_parts(niqki_group *g, Xbuf send, nqg::RecvBuf recv, size_t bytes, bool own_part) {
  if (g->transport == niqki_group::kRccl) {
    RcclGroupScope grp;
    NQ_GN(g, grp.begin());
    for (uint32_t l = 0; l < g->n_local; ++l) {
      NQ_GH(g, hipSetDevice(g->sh[l]->device));   // (several communicators in one thread: each call on its own device)
      const char *s = (const char *)g->ws[l].xbuf[send].p;
      char *r = (char *)(g->ws[l].*recv).p;
      if (!own_part) {
        NQ_GN(g, rccl().AllGather(s, r, bytes, ncclUint8, g->tp->comm[l], g->sh[l]->stream));
        continue;
      }
      for (uint32_t p = 0; p < g->world; ++p) {
        NQ_GN(g, rccl().Send(s + (size_t)p * bytes, bytes, ncclUint8, (int)p, g->tp->comm[l], g->sh[l]->stream));
        NQ_GN(g, rccl().Recv(r + (size_t)p * bytes, bytes, ncclUint8, (int)p, g->tp->comm[l], g->sh[l]->stream));
      }
    }
    NQ_GN(g, grp.end());
    return NIQKI_OK;
  }
  if (g->transport == niqki_group::kIpc)
    return ipc_collective(g, send, [&]() -> int {
      nq::PeerSrc src{};
      for (uint32_t s = 0; s < g->world; ++s) src.p[s] = (const uint8_t *)g->tp->ipc.peer_buf[s][send];
      const uint32_t bx = (uint32_t)std::min<uint64_t>((bytes / 16 + 255) / 256, 1024);
      hipLaunchKernelGGL(nq::ipc_pull_kernel, dim3(std::max(bx, 1u), g->world), dim3(256), 0, g->sh[0]->stream, src,
                         (uint64_t)(own_part ? g->first * bytes : 0), (uint64_t)bytes, (uint8_t *)(g->ws[0].*recv).p);
      NQ_GH(g, hipGetLastError());
      return NIQKI_OK;
    });
  int rc = cross_wait(g);
  if (rc) return rc;
  for (uint32_t l = 0; l < g->n_local; ++l) {
    NQ_GH(g, hipSetDevice(g->sh[l]->device));
    for (uint32_t s = 0; s < g->n_local; ++s)
      NQ_GH(g, hipMemcpyAsync((char *)(g->ws[l].*recv).p + (size_t)s * bytes,
                              (const char *)g->ws[s].xbuf[send].p + (own_part ? (size_t)l * bytes : 0), bytes,
                              hipMemcpyDeviceToDevice, g->sh[l]->stream));
  }
  return cross_wait(g);
}

}  // namespace

namespace nqg {

int all_to_all(niqki_group *g, Xbuf send, RecvBuf recv, size_t bytes) { return exchange_parts(g, send, recv, bytes, true); }
int all_gather(niqki_group *g, Xbuf send, RecvBuf recv, size_t bytes) { return exchange_parts(g, send, recv, bytes, false); }

int reduce_scatter_u32(niqki_group *g, Xbuf send, RecvBuf recv, size_t count) {
  if (g->transport == niqki_group::kRccl) {
    RcclGroupScope grp;
    NQ_GN(g, grp.begin());
    for (uint32_t l = 0; l < g->n_local; ++l) {
      NQ_GH(g, hipSetDevice(g->sh[l]->device));
      NQ_GN(g, rccl().ReduceScatter(g->ws[l].xbuf[send].p, (g->ws[l].*recv).p, count, ncclUint32, ncclSum, g->tp->comm[l], g->sh[l]->stream));
    }
    NQ_GN(g, grp.end());
    return NIQKI_OK;
  }
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((count + 255) / 256, 8192);
  if (g->transport == niqki_group::kIpc)
    return ipc_collective(g, send, [&]() -> int {
      if (count == 0) return NIQKI_OK;
      nq::SumSrc src{};
      for (uint32_t s = 0; s < g->world; ++s) src.p[s] = (const uint32_t *)g->tp->ipc.peer_buf[s][send];
      hipLaunchKernelGGL(nq::sum_rows_kernel, dim3(blocks), dim3(256), 0, g->sh[0]->stream, src, g->world, (uint64_t)g->first * count,
                         (uint64_t)count, (uint32_t *)(g->ws[0].*recv).p);
      NQ_GH(g, hipGetLastError());
      return NIQKI_OK;
    });
  int rc = cross_wait(g);
  if (rc) return rc;
  nq::SumSrc src{};
  for (uint32_t s = 0; s < g->n_local; ++s) src.p[s] = (const uint32_t *)g->ws[s].xbuf[send].p;
  for (uint32_t l = 0; l < g->n_local; ++l) {
    NQ_GH(g, hipSetDevice(g->sh[l]->device));
    if (count == 0) continue;
    hipLaunchKernelGGL(nq::sum_rows_kernel, dim3(blocks), dim3(256), 0, g->sh[l]->stream, src, g->world, (uint64_t)l * count,
                       (uint64_t)count, (uint32_t *)(g->ws[l].*recv).p);
    NQ_GH(g, hipGetLastError());
  }
  return cross_wait(g);
}

int reserve(niqki_group *g, const size_t need[kXbufs]) { return g->transport == niqki_group::kIpc ? ipc_prepare(g, need) : NIQKI_OK; }

int before_write(niqki_group *g, Xbuf b) {
  if (g->transport != niqki_group::kIpc) return NIQKI_OK;
  NQ_GH(g, hipSetDevice(g->sh[0]->device));
  return ipc_wait_all(g, kFlagDone + (uint32_t)b, g->tp->ipc.seq[b]);
}

int new_id(uint8_t *id) {
  static_assert(NIQKI_GROUP_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "group id is an ncclUniqueId");
  const char *t = std::getenv("NIQKI_GROUP_TRANSPORT");
  if (t && !std::strcmp(t, "ipc")) {   // no RCCL involved: 128 random bytes name the group
    FILE *f = std::fopen("/dev/urandom", "rb");
    const bool ok = f && std::fread(id, 1, NIQKI_GROUP_ID_BYTES, f) == NIQKI_GROUP_ID_BYTES;
    if (f) std::fclose(f);
    return ok ? NIQKI_OK : NIQKI_E_STATE;
  }
  if (!rccl().load()) return NIQKI_E_STATE;
  ncclUniqueId u;
  if (rccl().GetUniqueId(&u) != ncclSuccess) return NIQKI_E_HIP;
  std::memcpy(id, &u, NIQKI_GROUP_ID_BYTES);
  return NIQKI_OK;
}

int open(niqki_group *g, const uint8_t *id, bool shared_device) {
  const uint32_t n_local = g->n_local, world = g->world;
  g->tp = new (std::nothrow) niqki_group_transport();
  if (!g->tp) return gfail(g, NIQKI_E_NOMEM, "out of memory");
  const char *tenv = std::getenv("NIQKI_GROUP_TRANSPORT");
  const bool want_ipc = tenv && !std::strcmp(tenv, "ipc"), want_local = tenv && !std::strcmp(tenv, "local");
  const bool want_rccl = tenv && !std::strcmp(tenv, "rccl");   // asked for by name: RCCL decides whether it takes the devices
  if (want_ipc && n_local == 1 && world > 1) g->transport = niqki_group::kIpc;
  else if (n_local == world && !want_rccl && (shared_device || want_local || want_ipc)) g->transport = niqki_group::kLocal;
  else g->transport = niqki_group::kRccl;
  if (g->transport != niqki_group::kIpc && shared_device && n_local != world && !want_rccl)
    return gfail(g, NIQKI_E_INVALID, "shards that share a device need all ranks in one process (or NIQKI_GROUP_TRANSPORT=ipc)");
  if (g->transport == niqki_group::kIpc && n_local != 1)
    return gfail(g, NIQKI_E_INVALID, "the ipc transport wants one rank per process (or all ranks in one: local)");
  for (uint32_t l = 0; l < n_local; ++l) {   // (what cross_wait records)
    if (hipSetDevice(g->sh[l]->device) != hipSuccess || hipEventCreateWithFlags(&g->ws[l].ev, hipEventDisableTiming) != hipSuccess)
      return gfail(g, NIQKI_E_HIP, "hipEventCreate failed");
  }
  if (g->transport == niqki_group::kRccl) {
    if (!rccl().load()) return gfail(g, NIQKI_E_STATE, rccl().why);
    ncclUniqueId u;
    if (id) std::memcpy(&u, id, NIQKI_GROUP_ID_BYTES);
    else if (n_local != world) return gfail(g, NIQKI_E_INVALID, "a group spanning several processes needs the id of niqki_group_new_id");
    else if (rccl().GetUniqueId(&u) != ncclSuccess) return gfail(g, NIQKI_E_HIP, "ncclGetUniqueId failed");
    g->tp->comm.assign(n_local, nullptr);
    ncclResult_t r = rccl().GroupStart();
    for (uint32_t l = 0; l < n_local && r == ncclSuccess; ++l) {
      if (hipSetDevice(g->sh[l]->device) != hipSuccess) { r = ncclUnhandledCudaError; break; }
      r = rccl().CommInitRank(&g->tp->comm[l], (int)world, u, (int)(g->first + l));
    }
    const ncclResult_t r2 = rccl().GroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return gfail(g, NIQKI_E_HIP, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r != ncclSuccess ? r : r2));
  } else if (g->transport == niqki_group::kIpc) {
    if (!id) return gfail(g, NIQKI_E_INVALID, "a group spanning several processes needs the id of niqki_group_new_id");
    return ipc_setup(g, id);
  }
  return NIQKI_OK;
}

void close(niqki_group *g) {
  if (!g->tp) return;
  if (g->transport == niqki_group::kIpc && g->tp->ipc.shm) {
    if (g->tp->ipc.ready) (void)ipc_barrier(g);   // nobody still reads my buffers (a dead peer costs the timeout)
    ipc_teardown(g);
  }
  for (uint32_t l = 0; l < g->n_local && l < g->ws.size(); ++l) {
    if (g->ws[l].ev) (void)hipEventDestroy(g->ws[l].ev);
    if (l < g->tp->comm.size() && g->tp->comm[l]) (void)rccl().CommDestroy(g->tp->comm[l]);
  }
  delete g->tp;
  g->tp = nullptr;
}

int ranks_seen(const niqki_group *g, uint64_t *n) {
  *n = g->n_local;
  if (g->transport == niqki_group::kRccl) {
    int c = 0;
    if (g->tp->comm.empty() || !g->tp->comm[0] || rccl().CommCount(g->tp->comm[0], &c) != ncclSuccess) return NIQKI_E_STATE;
    *n = (uint64_t)c;
  } else if (g->transport == niqki_group::kIpc) {
    *n = 0;
    for (uint32_t s = 0; s < g->world; ++s) *n += g->tp->ipc.peer_flags[s] ? 1 : 0;
  }
  return NIQKI_OK;
}

const uint32_t *timeout_flag(const niqki_group *g) { return g->transport == niqki_group::kIpc ? g->tp->ipc.flags + kFlagErr : nullptr; }
uint64_t ipc_words_kind(const niqki_group *g) { return g->tp->ipc.words_kind; }
uint64_t ipc_arena_fine(const niqki_group *g) { return g->tp->ipc.arena_fine ? 1 : 0; }

}  // namespace nqg
