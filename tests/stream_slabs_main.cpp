// Stand-alone check of the stream-slab rule (csrc/stream_slabs.h, the only include of the project): built by tests/test_native_abi.py with
// the host compiler and -fsanitize=address,undefined.  Streams are opaque pointers here: the addresses of a few local bytes.
// Exit status 0 and "ok" when every property holds, else the failed line.
#include "../dinov2_od_amd/csrc/stream_slabs.h"

#include <cstdio>

#define CHECK(x) do { if (!(x)) { std::printf("stream_slabs_main.cpp:%d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
  char streams[6];      // six distinct addresses; &streams[i] is stream i
  StreamSlabs<4> s;

  // one stream keeps its slot across calls (the null stream included: `used`, not `owner`, marks a slot as taken)
  const int a = s.pick(&streams[0]);
  CHECK(a >= 0 && a < 4);
  CHECK(s.pick(&streams[0]) == a && s.pick(&streams[0]) == a);
  const int n = s.pick(nullptr);
  CHECK(n != a && s.pick(nullptr) == n);
  s.reset();

  // four distinct streams get four distinct slots, and keep them in any order of use
  int slot[4];
  bool seen[4] = {};
  for (int i = 0; i < 4; ++i) {
    slot[i] = s.pick(&streams[i]);
    CHECK(slot[i] >= 0 && slot[i] < 4 && !seen[slot[i]]);
    seen[slot[i]] = true;
  }
  for (int i = 3; i >= 0; --i) CHECK(s.pick(&streams[i]) == slot[i]);

  // a fifth evicts the least recently used: after the reversed round above that is stream 3, then stream 2
  CHECK(s.pick(&streams[4]) == slot[3]);
  CHECK(s.pick(&streams[0]) == slot[0] && s.pick(&streams[1]) == slot[1] && s.pick(&streams[2]) == slot[2]);
  CHECK(s.pick(&streams[4]) == slot[3]);            // the newcomer owns the slot now
  CHECK(s.pick(&streams[3]) == slot[0]);            // the evicted stream is a newcomer itself: it takes the oldest, stream 0's
  CHECK(s.pick(&streams[5]) == slot[1]);

  // reset() forgets owners: the next streams are handed slots from the first on, whoever held them
  s.reset();
  for (int i = 0; i < 4; ++i) CHECK(s.used[i] == 0 && s.owner[i] == nullptr);
  CHECK(s.pick(&streams[5]) == 0 && s.pick(&streams[4]) == 1 && s.pick(&streams[5]) == 0 && s.pick(&streams[2]) == 2);

  std::printf("ok\n");
  return 0;
}
