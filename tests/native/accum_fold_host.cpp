// Host driver for tests/test_accum_fold.py: accum_fold::fold128 (janus_amd/csrc/accum_fold.h, the
// end of k_accum_spec) behind a text protocol.  One tuple per input line,
//   ALO AHI BLO BHI     (hex, 64 bits each)
// -> one line with the folded element as 32 hex digits.
#include <inttypes.h>
#include <stdio.h>

#include "../../janus_amd/csrc/accum_fold.h"

int main() {
  uint64_t alo, ahi, blo, bhi;
  for (;;) {
    const int got = scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &alo, &ahi, &blo, &bhi);
    if (got == EOF) return 0;
    if (got != 4) {
      fprintf(stderr, "accum_fold_host: expected four hex words\n");
      return 2;
    }
    const accum_fold::u128 t = accum_fold::fold128(alo, ahi, blo, bhi);
    printf("%016" PRIx64 "%016" PRIx64 "\n", (uint64_t)(t >> 64), (uint64_t)t);
  }
}
