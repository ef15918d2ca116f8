// Runs scripted timer sequences over the profiling timers' event-pair bookkeeping
// (expecto_amd/csrc/event_pairs.h), the way beluga.hip's Timer and resolve_events use it, and prints
// what happened, for tests/test_event_pairs.py.
// stdin: one case per line: the pool's pairs, then ops: L (a layer timer opens), G (a launch timer
// opens), c (the innermost open timer closes), R (a resolve from outside, as layer_times does).
// stdout per case: "case", then per event one line:
//   open <serial> <pair>            resolve <timers open>       grow <timers open> <pairs after>
//   close <serial> <pair>           sample <layer|launch> <serial> <pair>   (the resolve's readings)
// then "end".  <serial> numbers the timers of the case in opening order.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../expecto_amd/csrc/event_pairs.h"

using namespace expecto;

struct Sample {
  int serial, pair;
  bool launch;
};

int main() {
  std::string ln;
  while (std::getline(std::cin, ln)) {
    std::istringstream is(ln);
    size_t pairs = 0;
    is >> pairs;
    EventPairs ev;
    ev.grow(pairs);
    std::vector<Sample> open, pending, pending_launch;
    int serial = 0;
    auto resolve = [&]() {
      std::printf("resolve %zu\n", ev.open_timers());
      for (const Sample& s : pending) std::printf("sample layer %d %d\n", s.serial, s.pair);
      pending.clear();
      for (const Sample& s : pending_launch) std::printf("sample launch %d %d\n", s.serial, s.pair);
      pending_launch.clear();
      ev.reset();
    };
    std::printf("case\n");
    for (std::string op; is >> op;) {
      if (op == "L" || op == "G") {
        const EventPairs::Room room = ev.room();
        if (room == EventPairs::Room::kResolve) resolve();
        if (room == EventPairs::Room::kGrow) {
          ev.grow(1);
          std::printf("grow %zu %zu\n", ev.open_timers(), ev.capacity());
        }
        const Sample s{serial++, ev.open(), op == "G"};
        std::printf("open %d %d\n", s.serial, s.pair);
        if (s.pair >= 0) open.push_back(s);
      } else if (op == "c") {
        const Sample s = open.back();
        open.pop_back();
        ev.close();
        std::printf("close %d %d\n", s.serial, s.pair);
        (s.launch ? pending_launch : pending).push_back(s);
      } else if (op == "R") {
        resolve();
      }
    }
    std::printf("end\n");
  }
  return 0;
}
