// Driver of tests/test_request_parse.py: janus_amd/csrc/request_parse.h (the per-report parser
// and fault rule the GPU kernels of helper_request.h run) built for the host.  A text protocol
// on stdin / stdout, one answer line per command:
//   pt <want> <hex | ->      -> "<status> <payload offset>" of parse_plaintext_input_share; the
//                               plaintext is parsed from a heap block of exactly its length, so
//                               a sanitizer build sees any read past it
//   fault <public_len> <prep_len> <message_type> <want_public> <want_prep>  -> prepare_init_fault
//   apply <status> <fault>   -> apply_fault
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "../../janus_amd/csrc/request_parse.h"

static int nib(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "pt") {
      uint32_t want = 0;
      std::string hex;
      in >> want >> hex;
      if (hex == "-") hex.clear();
      const size_t len = hex.size() / 2;
      std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);
      bool bad = hex.size() % 2 != 0;
      for (size_t i = 0; i < len && !bad; ++i) {
        const int h = nib(hex[2 * i]), l = nib(hex[2 * i + 1]);
        bad = h < 0 || l < 0;
        buf[i] = (uint8_t)(h * 16 + l);
      }
      if (bad) {
        std::printf("err bad hex\n");
        continue;
      }
      const p3g::PlaintextParse r = p3g::parse_plaintext_input_share(buf.get(), len, want);
      std::printf("%u %u\n", (unsigned)r.status, (unsigned)r.payload_off);
    } else if (cmd == "fault") {
      uint32_t a = 0, b = 0, t = 0, wa = 0, wb = 0;
      in >> a >> b >> t >> wa >> wb;
      std::printf("%u\n", (unsigned)p3g::prepare_init_fault(a, b, (uint8_t)t, wa, wb));
    } else if (cmd == "apply") {
      unsigned s = 0, f = 0;
      in >> s >> f;
      std::printf("%u\n", (unsigned)p3g::apply_fault((uint8_t)s, (uint8_t)f));
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
