// Strip geometry of the conv vector field (lrnde_conv.hip), host-includable so that tests/conv_geom_host.cpp and
// tests/conv_geometry_cases.py can be held to the function the kernels use.
//
// Every image is cut into strips of TR rows: TR is the largest divisor of H with TR*W <= maxpx pixels, 1 where no
// divisor fits (W <= maxpx is checked by lrnde_conv_create).  A strip has TP = TR*W pixels in MT = ceil(TP/16) M tiles.
#pragma once

inline int conv_strip_rows(int W, int H, int maxpx) {
  int best = 1;
  for (int tr = 1; tr <= H; ++tr)
    if (H % tr == 0 && tr * W <= maxpx) best = tr;
  return best;
}
