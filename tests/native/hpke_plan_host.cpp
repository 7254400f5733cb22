// Host driver for tests/test_hpke_plan.py: janus_amd/csrc/plan_hpke.h behind a text protocol, one
// command per input line.  KEYS = NT NG, then per key "ID KEM KDF AEAD SKLEN PKLEN SKP PKP" (SKP /
// PKP 0: a null pointer); every key points at the same bytes, so only its address tells it apart.
// REPORTS = N, then per report "CONFIG_ID STATUS ENC_LEN PAYLOAD_LEN".
//   plan OPT STRICT KEYS REPORTS -> lines route (F failed, U unknown, H host, or the group),
//       groups (key index, global keys after task keys), task, idx, gbeg, retry, offsets
//   fallback OPT WANT KEYS REPORTS s_0 .. s_{N-1}   (request mode; s: the device status image)
//       -> lines host, retry (report indices), layout KF O_ROWS O_ST BYTES, fb HEX, with
//          rows[i][b] = (7 i + 3 b + 1) & 255 and st[i] = (5 i + 2) & 255
//   info SENDER RECIPIENT -> the 20 bytes in hex
//   span OFF LEN TOTAL -> 0 / 1
//   blocks PUBLIC_SHARE_LEN PREP_SHARE_LEN N -> req_gather_blocks
//   views PUBLIC_SHARE_LEN PREP_SHARE_LEN MSG_LEN N K, then K x "INDEX REPORT_ID_OFF
//       PUBLIC_SHARE_OFF PUBLIC_SHARE_LEN ENC_OFF ENC_LEN PAYLOAD_OFF PAYLOAD_LEN PREP_SHARE_OFF
//       PREP_SHARE_LEN PREP_MSG_OFF PREP_MSG_LEN" (the other views are all zero)
//       -> "ok" or "err CODE MESSAGE"
//   suites OPTS KEM KDF AEAD -> "G T S": hpke_gpu_suite, hpke_team_suite, hpke_seal_suite (0 / 1)
//   columns KEM SHARE_LEN ENC_PITCH PAYLOAD_PITCH SHARE_PITCH -> share_columns: "NENC PLEN
//       ENC_PITCH PAYLOAD_PITCH SHARE_PITCH ENC_OK PAYLOAD_OK SHARE_OK OK"
//   rows N PITCH WIDTH -> rows_span
#include <stdio.h>

#include <iostream>
#include <sstream>

#include "../../janus_amd/csrc/plan_hpke.h"

using namespace p3g;

static const uint8_t kKeyBytes[65] = {1, 2, 3};

struct Input {
  std::vector<prio3gpu_hpke_keypair> keys;
  size_t nt = 0, ng = 0;
  std::vector<prio3gpu_prepare_init_view> views;
  std::vector<uint8_t> status;
  const prio3gpu_hpke_keypair* task() const { return nt ? keys.data() : nullptr; }
  const prio3gpu_hpke_keypair* global() const { return ng ? keys.data() + nt : nullptr; }
};

static Input read_input(std::istream& in) {
  Input x;
  in >> x.nt >> x.ng;
  x.keys.resize(x.nt + x.ng);
  for (auto& k : x.keys) {
    unsigned id, kem, kdf, aead, skp, pkp;
    in >> id >> kem >> kdf >> aead >> k.private_key_len >> k.public_key_len >> skp >> pkp;
    k.config_id = (uint8_t)id, k.kem_id = (uint16_t)kem, k.kdf_id = (uint16_t)kdf;
    k.aead_id = (uint16_t)aead;
    k.private_key = skp ? kKeyBytes : nullptr;
    k.public_key = pkp ? kKeyBytes : nullptr;
  }
  size_t n;
  in >> n;
  x.views.assign(n, prio3gpu_prepare_init_view{});
  x.status.resize(n);
  for (size_t i = 0; i < n; ++i) {
    unsigned id, st;
    in >> id >> st >> x.views[i].enc_len >> x.views[i].payload_len;
    x.views[i].hpke_config_id = (uint8_t)id, x.status[i] = (uint8_t)st;
  }
  return x;
}

static HpkePlan make_plan(const Input& x, bool opt, bool strict) {
  HpkePlan p;
  plan_hpke(x.task(), x.nt, x.global(), x.ng, x.views.data(), x.status.data(), x.views.size(), opt,
            strict, &p);
  return p;
}

template <class V>
static void print_vec(const char* name, const V& v) {
  printf("%s", name);
  for (auto e : v) printf(" %llu", (unsigned long long)e);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "plan") {
      int opt, strict;
      in >> opt >> strict;
      const Input x = read_input(in);
      const size_t n = x.views.size();
      const HpkePlan p = make_plan(x, opt != 0, strict != 0);
      printf("route");
      for (int32_t r : p.route) {
        if (r >= 0) printf(" %d", r);
        else printf(" %c", r == ROUTE_FAILED ? 'F' : r == ROUTE_UNKNOWN ? 'U' : 'H');
      }
      printf("\ngroups");
      for (const prio3gpu_hpke_keypair* kp : p.groups) printf(" %td", kp - x.keys.data());
      printf("\n");
      print_vec("task", p.is_task_key);
      print_vec("idx", p.idx);
      print_vec("gbeg", p.gbeg);
      std::vector<int> retry(n);
      for (size_t i = 0; i < n; ++i) retry[i] = wants_global_retry(p, x.views.data(), i);
      print_vec("retry", retry);
      std::vector<uint64_t> off(n + 1);
      plaintext_offsets(x.views.data(), n, off.data());
      print_vec("offsets", off);
    } else if (cmd == "fallback") {
      int opt;
      uint32_t want;
      in >> opt >> want;
      const Input x = read_input(in);
      const size_t n = x.views.size();
      const HpkePlan p = make_plan(x, opt != 0, false);
      std::vector<uint8_t> image(n), rows(n * (size_t)want), st(n), fb;
      for (size_t i = 0; i < n; ++i) {
        unsigned s;
        in >> s;
        image[i] = (uint8_t)s, st[i] = (uint8_t)(5 * i + 2);
        for (uint32_t b = 0; b < want; ++b) rows[i * want + b] = (uint8_t)(7 * i + 3 * b + 1);
      }
      HpkeFallback f;
      classify_fallback(p, x.views.data(), image.data(), n, &f);
      std::vector<size_t> host, retry;
      for (size_t i = 0; i < n; ++i) {
        if (!f.st_host[i]) host.push_back(i);
        if (!f.st_retry[i]) retry.push_back(i);
      }
      if (host.size() != f.n_host || retry.size() != f.n_retry) printf("err counts\n");
      print_vec("host", host);
      print_vec("retry", retry);
      const FallbackLayout l = pack_fallback(f, n, rows.data(), st.data(), want, &fb);
      printf("layout %zu %zu %zu %zu\nfb ", l.kf, l.o_rows, l.o_st, l.bytes);
      for (uint8_t b : fb) printf("%02x", b);
      printf("\n");
    } else if (cmd == "info") {
      unsigned s, r;
      in >> s >> r;
      uint8_t info[20];
      input_share_info((uint8_t)s, (uint8_t)r, info);
      for (uint8_t b : info) printf("%02x", b);
      printf("\n");
    } else if (cmd == "span") {
      uint64_t off, len, total;
      in >> off >> len >> total;
      printf("%d\n", (int)span_fits(off, len, total));
    } else if (cmd == "suites") {
      unsigned opts, kem, kdf, aead;
      in >> opts >> kem >> kdf >> aead;
      printf("%d %d %d\n", (int)hpke_gpu_suite(opts, (uint16_t)kem, (uint16_t)kdf, (uint16_t)aead),
             (int)hpke_team_suite(opts, (uint16_t)kem, (uint16_t)kdf, (uint16_t)aead),
             (int)hpke_seal_suite(opts, (uint16_t)kem, (uint16_t)kdf, (uint16_t)aead));
    } else if (cmd == "columns") {
      unsigned kem;
      uint32_t share_len;
      uint64_t ep, pp, sp;
      in >> kem >> share_len >> ep >> pp >> sp;
      const ShareColumns g = share_columns((uint16_t)kem, share_len, ep, pp, sp);
      printf("%llu %llu %llu %llu %llu %d %d %d %d\n", (unsigned long long)g.nenc,
             (unsigned long long)g.plen, (unsigned long long)g.enc_pitch,
             (unsigned long long)g.payload_pitch, (unsigned long long)g.share_pitch,
             (int)g.enc_ok, (int)g.payload_ok, (int)g.share_ok, (int)g.ok());
    } else if (cmd == "rows") {
      uint64_t n, pitch, width;
      in >> n >> pitch >> width;
      printf("%llu\n", (unsigned long long)rows_span(n, pitch, width));
    } else if (cmd == "blocks" || cmd == "views") {
      Cfg g{};
      in >> g.public_share_len >> g.prep_share_len;
      size_t msg_len = 0, n, k = 0;
      if (cmd == "views") in >> msg_len;
      in >> n;
      if (cmd == "blocks") {
        printf("%llu\n", (unsigned long long)req_gather_blocks(g, n));
        continue;
      }
      in >> k;
      std::vector<prio3gpu_prepare_init_view> views(n, prio3gpu_prepare_init_view{});
      for (size_t j = 0; j < k; ++j) {
        size_t i;
        in >> i;
        prio3gpu_prepare_init_view& v = views[i];
        in >> v.report_id_off >> v.public_share_off >> v.public_share_len >> v.enc_off >>
            v.enc_len >> v.payload_off >> v.payload_len >> v.prep_share_off >> v.prep_share_len >>
            v.prep_msg_off >> v.prep_msg_len;
      }
      std::string err;
      const int rc = check_request_views(g, views.data(), n, msg_len, &err);
      if (rc) printf("err %d %s\n", rc, err.c_str());
      else printf("ok\n");
    } else {
      printf("err unknown command\n");
    }
  }
  return 0;
}
