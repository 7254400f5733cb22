// Host driver for tests/test_hpke_plan_p256.py: janus_amd/csrc/plan_hpke.h with the option mask
// (HPKE_OPT_SUITES = 1, HPKE_OPT_P256 = 2) and real key bytes, which a P-256 keypair needs to pass
// the host's validation.  One command per input line:
//   plan OPTS STRICT NT NG, then per key "ID KEM KDF AEAD SKHEX PKHEX" ("-": empty), then N and per
//       report "CONFIG_ID STATUS ENC_LEN PAYLOAD_LEN"
//       -> "route ..." (F failed, U unknown, H host, or the group) and "groups ..." (key indices,
//          global keys after task keys)
//   scalar SKHEX -> p256_scalar_valid as 0 / 1
#include <stdio.h>

#include <iostream>
#include <sstream>

#include "../../janus_amd/csrc/plan_hpke.h"

using namespace p3g;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  out.shrink_to_fit();
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "plan") {
      unsigned opts, strict;
      size_t nt, ng, n;
      in >> opts >> strict >> nt >> ng;
      std::vector<prio3gpu_hpke_keypair> keys(nt + ng);
      std::vector<std::vector<uint8_t>> sks(nt + ng), pks(nt + ng);
      for (size_t k = 0; k < keys.size(); ++k) {
        unsigned id, kem, kdf, aead;
        std::string sk, pk;
        in >> id >> kem >> kdf >> aead >> sk >> pk;
        sks[k] = unhex(sk), pks[k] = unhex(pk);
        keys[k].config_id = (uint8_t)id, keys[k].kem_id = (uint16_t)kem;
        keys[k].kdf_id = (uint16_t)kdf, keys[k].aead_id = (uint16_t)aead;
        keys[k].private_key = sks[k].empty() ? nullptr : sks[k].data();
        keys[k].private_key_len = sks[k].size();
        keys[k].public_key = pks[k].empty() ? nullptr : pks[k].data();
        keys[k].public_key_len = pks[k].size();
      }
      in >> n;
      std::vector<prio3gpu_prepare_init_view> views(n, prio3gpu_prepare_init_view{});
      std::vector<uint8_t> status(n);
      for (size_t i = 0; i < n; ++i) {
        unsigned id, st;
        in >> id >> st >> views[i].enc_len >> views[i].payload_len;
        views[i].hpke_config_id = (uint8_t)id, status[i] = (uint8_t)st;
      }
      HpkePlan p;
      plan_hpke(nt ? keys.data() : nullptr, nt, ng ? keys.data() + nt : nullptr, ng, views.data(),
                status.data(), n, opts, strict != 0, &p);
      printf("route");
      for (int32_t r : p.route) {
        if (r >= 0) printf(" %d", r);
        else printf(" %c", r == ROUTE_FAILED ? 'F' : r == ROUTE_UNKNOWN ? 'U' : 'H');
      }
      printf("\ngroups");
      for (const prio3gpu_hpke_keypair* kp : p.groups) printf(" %td", kp - keys.data());
      printf("\n");
    } else if (cmd == "scalar") {
      std::string sk;
      in >> sk;
      const std::vector<uint8_t> b = unhex(sk);
      printf("%d\n", b.size() == 32 && p256_scalar_valid(b.data()) ? 1 : 0);
    } else if (!cmd.empty()) {
      printf("err unknown command\n");
    }
  }
  return 0;
}
