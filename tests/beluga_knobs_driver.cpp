// Prints the handle knobs (expecto_amd/csrc/beluga_knobs.h) parsed from a given environment, for
// tests/test_beluga_knobs.py.
// stdin: one case per line, whitespace-separated NAME=VALUE settings (an empty line: no variable set).
// stdout per case: "case", then "error <refusal>" or one "<variable> <value of its field>" line per
// knob of the table; then "end".
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../expecto_amd/csrc/beluga_knobs.h"

using namespace expecto;

int main() {
  std::string ln;
  while (std::getline(std::cin, ln)) {
    std::map<std::string, std::string> env;
    std::istringstream is(ln);
    for (std::string kv; is >> kv;) env[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
    BelugaKnobs k;
    const char* err = beluga_knobs_parse(k, [&](const char* name) -> const char* {
      const auto it = env.find(name);
      return it == env.end() ? nullptr : it->second.c_str();
    });
    std::printf("case\n");
    if (err) {
      std::printf("error %s\nend\n", err);
      continue;
    }
    for (const BelugaKnob& s : kBelugaKnobs) {
      if (s.b)
        std::printf("%s %d\n", s.name, (int)(k.*s.b));
      else if (s.d)
        std::printf("%s %.17g\n", s.name, k.*s.d);
      else
        std::printf("%s %d\n", s.name, k.*s.i);
    }
    std::printf("end\n");
  }
  return 0;
}
