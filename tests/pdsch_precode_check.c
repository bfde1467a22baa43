/* Stand-alone check of the precoding arithmetic of csrc/nr_pdsch_map.h (tests/test_pdsch_precode_host.py compiles and runs it, with
 * the host sanitizers):   pdsch_precode_check Nl pmi ant m0 m1 m2 m3 w0 w1 w2 w3 [the same eleven again ...]
 * m = the layers' mapped values, w = the antenna's weights, c16 words in hex (r in the low half).  Prints nr_pdm_antenna of each
 * group as a hex word, one a line.  The library reaches a mapped value of -32768 with no amp, this program does. */
#include <stdio.h>
#include <stdlib.h>
#include "nr_pdsch_map.h"

int main(int argc, char **argv)
{
  if (argc < 12 || (argc - 1) % 11 != 0) {
    fprintf(stderr, "usage: pdsch_precode_check Nl pmi ant m0 m1 m2 m3 w0 w1 w2 w3 ...\n");
    return 2;
  }
  for (int a = 1; a + 10 < argc; a += 11) {
    uint32_t v[11];
    for (int k = 0; k < 11; k++)
      v[k] = (uint32_t)strtoul(argv[a + k], NULL, 16);
    if (v[0] < 1 || v[0] > NR_PDM_MAX_LAYERS || v[2] >= NR_PDM_MAX_TX)
      return 2;
    printf("%08x\n", nr_pdm_antenna(v + 3, v + 7, v[0], v[2], v[1]));
  }
  return 0;
}
