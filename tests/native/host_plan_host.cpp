// Host driver for tests/test_host_plan.py: the engine's HIP-free planning headers behind a text
// protocol, one command per input line, one or more output lines each:
//   cfg K BITS LEN CHUNK      -> "ok" + Cfg lengths + prio3gpu_sizes fields, or "err MESSAGE"
//   spec K BITS LEN CHUNK     -> "ok ND E0 E1" or "none"
//   chunks LO HI              -> optimal_chunk_length(LO..HI) on one line
//   gadget M CALLS ES         -> the 3M + 1 table entries (Montgomery form) in hex
//   prover M ES               -> the 2M + 2 table entries in hex
//   accum N S MEAS_LEN SPEC K s_0 .. s_{K-1}   (K = 0: no per-report slots, else K = N)
//       -> "ok NDIR NSPEC NCH CH WCH", then one line per array (perm, cb, cs, dir, sid, swb, wl),
//          then "layout" + the AccumLayout fields; or "err MESSAGE"
#include <stdio.h>

#include <iostream>
#include <sstream>

#include "../../janus_amd/csrc/cfg.h"
#include "../../janus_amd/csrc/plan_accum.h"
#include "../../janus_amd/csrc/plan_cfg.h"

using namespace p3g;

static void print_table(const std::vector<uint8_t>& t, uint32_t es) {
  for (size_t k = 0; k < t.size() / es; ++k) {
    for (uint32_t b = es; b-- > 0;) printf("%02x", t[k * es + b]);
    printf(k + 1 < t.size() / es ? " " : "\n");
  }
}

static void print_vec(const char* name, const std::vector<uint32_t>& v) {
  printf("%s", name);
  for (uint32_t x : v) printf(" %u", x);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "cfg" || cmd == "spec") {
      int kind;
      uint32_t bits, length, chunk;
      in >> kind >> bits >> length >> chunk;
      Cfg g;
      std::string err;
      if (derive_cfg(kind, bits, length, chunk, &g, &err)) {
        printf("err %s\n", err.c_str());
      } else if (cmd == "spec") {
        uint32_t nd = 0, e0 = 0, e1 = 0;
        if (spec_range(g, nd, e0, e1)) printf("ok %u %u %u\n", nd, e0, e1);
        else printf("none\n");
      } else {
        const prio3gpu_sizes s = cfg_sizes(g);
        printf("ok %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", g.es, g.meas_len, g.proof_len,
               g.verifier_len, g.jr_len, g.out_len, g.prove_rand_len, g.leader_share_len,
               g.helper_share_len, g.public_share_len, g.prep_share_len, g.prep_msg_len, g.m,
               g.calls, g.chunk);
        printf(" %u %u %u %u %u %u %u %u %u %u %u %u\n", s.field_size, s.meas_len, s.proof_len,
               s.verifier_len, s.joint_rand_len, s.output_len, s.leader_input_share,
               s.helper_input_share, s.public_share, s.prep_share, s.prep_msg, s.aggregate_share);
      }
    } else if (cmd == "chunks") {
      uint32_t lo, hi;
      in >> lo >> hi;
      for (uint32_t l = lo; l <= hi; ++l) printf(l < hi ? "%u " : "%u\n", optimal_chunk_length(l));
    } else if (cmd == "gadget") {
      uint32_t m, calls, es;
      in >> m >> calls >> es;
      print_table(gadget_table(m, calls, es), es);
    } else if (cmd == "prover") {
      uint32_t m, es;
      in >> m >> es;
      print_table(prover_table(m, es), es);
    } else if (cmd == "accum") {
      size_t n, k;
      uint32_t S, meas_len;
      int spec;
      in >> n >> S >> meas_len >> spec >> k;
      std::vector<uint32_t> slots(k);
      for (auto& s : slots) in >> s;
      AccumPlan p;
      std::string err;
      if (plan_accumulate(n, k ? slots.data() : nullptr, S, meas_len, spec != 0, &p, &err)) {
        printf("err %s\n", err.c_str());
        continue;
      }
      printf("ok %u %u %u %zu %zu\n", p.ndir, p.nspec, p.nch, accum_direct_chunk(n, meas_len),
             kAccumWCH);
      print_vec("perm", p.perm);
      print_vec("cb", p.chunk_begin);
      print_vec("cs", p.chunk_slot);
      print_vec("dir", p.dir_ids);
      print_vec("sid", p.spec_ids);
      print_vec("swb", p.spec_wave_begin);
      print_vec("wl", p.wave_list);
      const AccumLayout l = accum_layout(p);
      printf("layout %zu %zu %zu %zu %zu %zu %zu %zu\n", l.chunk_begin, l.chunk_slot,
             l.chunks_len, l.dir_ids, l.spec_ids, l.spec_wave_begin, l.wave_list, l.spec_idx_len);
    } else {
      printf("err unknown command\n");
    }
  }
  return 0;
}
