// piece_reader.h -- lines mode's input side: a thread streams a FASTA / FASTQ file (plain or gzip) into page-locked
// pieces that end at a record boundary and hands them out in file order.  Also the small blocking queue the host
// program's threads pass buffers through.  Part of index_host.cpp's translation unit; no device code.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "file_reader.h"
#include "gzio.h"

namespace nqhost {
namespace {

// Small blocking queue for handing buffers between the stages.
template <typename T>
class Channel {
 public:
  void push(T v) {
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(std::move(v));
    }
    cv_.notify_all();
  }
  void push_front(T v) {   // the next one to be popped
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_front(std::move(v));
    }
    cv_.notify_all();
  }
  T pop() {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return !q_.empty(); });
    T v = std::move(q_.front());
    q_.pop_front();
    return v;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<T> q_;
};

// End of the last complete record in buf[0, size): the reader cuts its pieces there, so
// every piece holds whole records (the GPU frames them; this is only a safe place to cut).
// FASTA: a line that starts with '>' begins a record.  FASTQ: records are 4 lines, and a
// piece starts at a record, so the cut is after a multiple of 4 newlines.  0 = none yet.
size_t record_cut(const uint8_t *buf, size_t size, char type) {
  if (type == 'Q') {
    size_t lines = 0, cut = 0;
    const uint8_t *p = buf, *end = buf + size;
    while (p < end) {
      const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
      if (!nl) break;
      p = nl + 1;
      if ((++lines & 3) == 0) cut = (size_t)(p - buf);
    }
    return cut;
  }
  size_t hi = size;
  while (hi > 1) {
    const uint8_t *gt = (const uint8_t *)memrchr(buf + 1, '>', hi - 1);
    if (!gt) return 0;
    if (gt[-1] == '\n') return (size_t)(gt - buf);
    hi = (size_t)(gt - buf);
  }
  return 0;
}

// the header line that starts at base[at], without its newline (base holds `room` bytes)
std::string header_line(const uint8_t *base, size_t room, uint64_t at) {
  const uint8_t *b = base + at;
  const uint8_t *nl = (const uint8_t *)memchr(b, '\n', room - at);
  return std::string((const char *)b, nl ? (size_t)(nl - b) : (size_t)(room - at));
}

struct Piece {
  PinnedBuf buf;
  bool last = false;
  std::string err;
  std::atomic<int> refs{0};   // the GPU thread while it works on the piece + every batch of hits whose names still lie in it
};

// Six pieces go round: one being read, one on the GPU, up to four whose header lines the writer still needs.  next()
// hands out the file's pieces in order, each with one reference; whoever drops a piece's last reference (release)
// hands it back to the reader thread.
class PieceReader {
 public:
  PieceReader(const std::string &path, char type) : pieces_(6) {
    for (auto &pc : pieces_) free_.push(&pc);
    th_ = std::thread([this, path, type] { run(path, type); });
  }
  ~PieceReader() { stop(); }
  // the next piece (the file's last one has `last` set); a read error is thrown here
  Piece *next() {
    Piece *pc = ready_.pop();
    pc->refs.store(1);
    if (!pc->err.empty()) throw std::runtime_error(pc->err);
    return pc;
  }
  void retain(Piece *pc) { pc->refs.fetch_add(1); }
  void release(Piece *pc) {
    if (pc->refs.fetch_sub(1) == 1) free_.push(pc);
  }
  void stop() {   // also releases a reader that waits for a piece nobody will hand back
    free_.push(nullptr);
    if (th_.joinable()) th_.join();
  }

 private:
  void run(const std::string &path, char type) {
    std::vector<uint8_t> carry;   // the unfinished record behind the last cut: the head of the next piece
    size_t target = size_t(8) << 20;
    bool eof = false;
    try {
      GzReader in(path);
      while (!eof) {
        Piece *pc = free_.pop();
        if (!pc) return;  // the consumer gave up
        pc->err.clear();
        pc->last = false;
        pc->buf.size = 0;
        pc->buf.reserve(std::max(target, carry.size()) + (size_t(1) << 16));
        if (!carry.empty()) std::memcpy(pc->buf.p, carry.data(), carry.size());   // (an empty vector's data() may be null)
        pc->buf.size = carry.size();
        carry.clear();
        size_t cut = 0;
        for (;;) {
          while (!eof && pc->buf.size < target) {
            const size_t n = in.read(pc->buf.p + pc->buf.size, target - pc->buf.size);
            pc->buf.size += n;
            if (n == 0 || in.eof()) eof = true;
          }
          if (eof) { cut = pc->buf.size; break; }
          cut = record_cut(pc->buf.p, pc->buf.size, type);
          if (cut) break;
          target *= 2;  // not one complete record yet: a longer piece
          pc->buf.reserve(target + (size_t(1) << 16));
        }
        carry.assign(pc->buf.p + cut, pc->buf.p + pc->buf.size);
        pc->buf.size = cut;
        pc->last = eof;
        ready_.push(pc);
      }
    } catch (const std::exception &e) {
      Piece *pc = free_.pop();
      if (pc) { pc->err = e.what(); pc->last = true; pc->buf.size = 0; ready_.push(pc); }
    }
  }

  std::deque<Piece> pieces_;
  Channel<Piece *> free_, ready_;
  std::thread th_;
};

}  // namespace
}  // namespace nqhost
