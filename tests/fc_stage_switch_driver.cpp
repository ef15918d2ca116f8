// Prints what the handle's knob parser (expecto_amd/csrc/beluga_knobs.h) makes of the FC stage's
// settings, for tests/test_fc_stage_plan.py.  argv: NAME=VALUE settings (none: nothing set).
// stdout: "error <refusal>", or "fk_slice <n>" and "fk_alt_inplace <0/1>".
#include <cstdio>
#include <map>
#include <string>

#include "../expecto_amd/csrc/beluga_knobs.h"

int main(int argc, char** argv) {
  std::map<std::string, std::string> env;
  for (int i = 1; i < argc; ++i) {
    const std::string kv = argv[i];
    env[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
  }
  expecto::BelugaKnobs k;
  const char* err = expecto::beluga_knobs_parse(k, [&](const char* name) -> const char* {
    const auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  });
  if (err) {
    std::printf("error %s\n", err);
    return 0;
  }
  std::printf("fk_slice %d\nfk_alt_inplace %d\n", k.fk_slice, (int)k.fk_alt_inplace);
  return 0;
}
