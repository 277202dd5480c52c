// The strip geometry of the conv vector field as the kernels compute it: conv_strip_rows of csrc/lrnde_conv_geom.hpp,
// the function lrnde_conv.hip calls for the forward strips and for the weight-gradient strips (maxpx = 16 * MAXMT = 128).
// tests/test_host_conv_geometry.py compares it with geometry() of tests/conv_geometry_cases.py.
//
//   conv_geom_host W H [W H ...]      prints one line "W H TR" per pair
#include "lrnde_conv_geom.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2 != 0) return 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const int W = atoi(argv[i]), H = atoi(argv[i + 1]);
    if (W < 1 || H < 1) return 2;
    printf("%d %d %d\n", W, H, conv_strip_rows(W, H, 128));
  }
  return 0;
}
