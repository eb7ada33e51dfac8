// Stand-alone check of csrc/rt_order.h (built and run by tests/test_order_paths_cpu.py with g++ -fsanitize=undefined,address): the node
// step without the sorting network (RT_ORDER_PATHS: path A, no more than one valid child) against the step with the network, restated
// here as rt_traverse_loop.inc performs it, on every output of the step: does the lane pop, the child it goes on with, the entries it
// pushes in order with their path maxima (none), and its new path maximum.
//
// Cases: all 16 validity masks x every assignment of the distances {-1, -0, +0, 1, 2} to the four slots (ties in every slot pair, the
// two zeros among them) x four path maxima in front of the step.  A slot that is not valid gets a distance that would win every
// comparison if it were read, and a descriptor that is nobody's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "rt_order.h"

struct Step {
  bool pop = false;
  uint32_t cur = 0;
  float path_m = 0;
  std::vector<Cand> pushed;   // in push order; d holds the entry's path maximum
};

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static bool same(const Step& a, const Step& b) {
  if (a.pop != b.pop) return false;
  if (a.pop) return true;
  if (a.cur != b.cur || bits(a.path_m) != bits(b.path_m) || a.pushed.size() != b.pushed.size()) return false;
  for (size_t i = 0; i < a.pushed.size(); ++i)
    if (a.pushed[i].desc != b.pushed[i].desc || bits(a.pushed[i].d) != bits(b.pushed[i].d)) return false;
  return true;
}

// the ordered arm as it stands behind the paths: +inf into the children that are not valid, the network, far children first
static Step network_step(const Cand* in, const bool* ok, float path_m) {
  Cand c[4];
  for (int k = 0; k < 4; ++k) { c[k] = in[k]; c[k].d = ok[k] ? c[k].d : INFINITY; }
  order_children(c);
  Step s;
  if (c[0].d < INFINITY) {
    for (int k = 3; k >= 1; --k) if (c[k].d < INFINITY) s.pushed.push_back(Cand{vmax_nonan(path_m, c[k].d), c[k].desc});
    s.cur = c[0].desc;
    s.path_m = vmax_nonan(path_m, c[0].d);
  } else s.pop = true;
  return s;
}

static Step path_a_step(const Cand* c, const bool* ok, float path_m) {
  Step s;
  if (order_any_valid(ok)) {
    const Cand n = order_first_valid(c, ok);
    s.cur = n.desc;
    s.path_m = vmax_nonan(path_m, n.d);
  } else s.pop = true;
  return s;
}

int main() {
  const float dist[5] = {-1.0f, -0.0f, 0.0f, 1.0f, 2.0f};
  const float maxima[4] = {-INFINITY, -0.0f, 0.5f, 3.0f};
  long cases = 0, a_cases = 0, failures = 0;
  for (int mask = 0; mask < 16; ++mask) {
    const bool ok[4] = {(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0};
    const int n = ok[0] + ok[1] + ok[2] + ok[3];
    if (order_any_valid(ok) != (n >= 1) || order_two_valid(ok) != (n >= 2) || order_three_valid(ok) != (n >= 3)) {
      std::printf("mask %d: the counting conditions disagree with %d valid children\n", mask, n);
      ++failures;
    }
    for (int a = 0; a < 625; ++a) {
      const int pick[4] = {a % 5, (a / 5) % 5, (a / 25) % 5, a / 125};
      Cand c[4];
      for (int k = 0; k < 4; ++k) {
        c[k].d = ok[k] ? dist[pick[k]] : -1000.0f - (float)pick[k];   // (never to be read where the slot is not valid)
        c[k].desc = ok[k] ? 0x100u + (uint32_t)k : 0xdead0000u + (uint32_t)k;
      }
      for (float pm : maxima) {
        ++cases;
        const Step want = network_step(c, ok, pm);
        if (n <= 1) {
          ++a_cases;
          if (!same(path_a_step(c, ok, pm), want)) { ++failures; std::printf("path A differs: mask %d distances %d path_m %g\n", mask, a, pm); }
        }
        // more than one valid child: the step keeps the network; what the test of the run must see is that such a lane is counted
        if (n >= 2 && !order_two_valid(ok)) { ++failures; std::printf("mask %d: a lane with %d valid children passes the test of path A\n", mask, n); }
        if (failures > 20) return 1;
      }
    }
  }
  std::printf("%ld cases, %ld through path A, %ld failures\n", cases, a_cases, failures);
  return failures ? 1 : 0;
}
