// Which slab of a small fixed set a launching stream gets: the slot bookkeeping of the stream-slab pools (gemm_dispatch.hip SlabPool).
// Plain C++ (a stream is an opaque pointer here), so the rule is tested on the host: tests/stream_slabs_main.cpp.
//
// Slabs go to launching streams least-recently-used first (a forward may run as concurrent micro-batches on separate streams -- engine.py:
// two -- and a process creates many short-lived streams over time: warm-up, capture, side streams).  Streams that launch concurrently must
// not share a slab: up to SLOTS of them never do.  More than SLOTS concurrent streams share slabs: known, and not handled.
#pragma once

template <int SLOTS>
struct StreamSlabs {
  const void* owner[SLOTS] = {};
  unsigned long long used[SLOTS] = {};      // clock value of the slot's last pick; 0 = never handed out (its owner means nothing)
  unsigned long long clock = 0;

  // the slot this stream already owns, else the least recently used one, which the stream then owns
  int pick(const void* stream) {
    int p = -1;
    for (int i = 0; i < SLOTS; ++i)
      if (used[i] && owner[i] == stream) { p = i; break; }
    if (p < 0) {
      p = 0;
      for (int i = 1; i < SLOTS; ++i)
        if (used[i] < used[p]) p = i;
      owner[p] = stream;
    }
    used[p] = ++clock;
    return p;
  }
  // forget every owner (the slabs moved: no stream's earlier slot means anything)
  void reset() {
    for (int i = 0; i < SLOTS; ++i) { used[i] = 0; owner[i] = nullptr; }
  }
};
