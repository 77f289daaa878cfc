// Test driver (not part of the product): the host-only hull plane builder of csrc/render_build.h on
// hulls from a file, with no GPU and no HIP - g++ alone compiles it (tests/test_render_build.py; by
// hand under -fsanitize=address,undefined).
// usage: render_build_check IN
//   IN: any number of hulls, each an int32 vertex count (1 .. PS_HULL_MAXVERT) and then that many
//   fp64 xyz triples. Per hull it prints "<return code> <message>" of build_hull_planes (the
//   device table's builder, with its cap), then the number of planes hull_planes found (-1: none)
//   and one line "nx ny nz off" per plane in fp64. Exit status 0 whenever the input could be read.
#include <stdio.h>

#include <string>
#include <vector>

#include "../diffusion-piano_amd/csrc/render_build.h"

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return fprintf(stderr, "usage: render_build_check IN\n"), 2;
  int32_t nv;
  while (fread(&nv, sizeof(nv), 1, f) == 1) {
    if (nv < 1 || nv > PS_HULL_MAXVERT) return fprintf(stderr, "vertex count out of range\n"), 2;
    std::vector<double> v((size_t)nv * 3);
    if (fread(v.data(), sizeof(double), v.size(), f) != v.size()) return fprintf(stderr, "short input\n"), 2;
    // the hull as extra collider 0 of a model with no other
    constexpr int NXT = PS_NHAND * PS_HAND_NXGEOM;
    int type[NXT] = {PS_GEOM_HULL}, v0[NXT] = {0}, cnt[NXT] = {nv};
    std::vector<float> plane;
    std::vector<int> count;
    std::string err;
    const int rc = psr::build_hull_planes(type, v0, cnt, v.data(), 3, plane, count, err);
    printf("%d %s\n", rc, err.c_str());
    std::vector<psr::Plane> pl;
    const int n = psr::hull_planes(reinterpret_cast<const double(*)[3]>(v.data()), nv, pl, err);
    printf("%d\n", n);
    for (int i = 0; i < n; i++) printf("%.17g %.17g %.17g %.17g\n", pl[i].n[0], pl[i].n[1], pl[i].n[2], pl[i].off);
  }
  fclose(f);
  return 0;
}
