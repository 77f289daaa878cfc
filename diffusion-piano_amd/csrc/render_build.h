// render_build.h - host-only: the face planes of a convex hull collider, for the ray caster
// (render.inc). A hull is the convex hull of its vertices (geom frame); a ray is clipped against
// the half spaces n . x <= off of its faces. Built once per handle, at its first ps_render.
//
// The builder tries the plane through every vertex triple and keeps the ones with every vertex on
// one side: O(V^4) for V <= PS_HULL_MAXVERT = 64 vertices, a few million multiply-adds per hull.
// Triples of one face give the same plane: coplanar facets are merged by dropping duplicates.
// No HIP here: tools/render_build_check.cpp compiles it with g++ alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pianosim.h"

namespace psr {

// The most face planes of one hull. The default hull fingertips have 50 vertices and 88 planes
// each; a hull of V vertices in general position has 2 V - 4 (124 at PS_HULL_MAXVERT).
constexpr int HULL_MAXPLANE = 96;

struct Plane {
  double n[3], off;  // unit outward normal; inside: n . x <= off
};

// a vertex is on a plane within this distance (m): the hulls are centimetres across and their
// vertices fp64, so rounding is ~1e-18; authored coplanar faces deviate by nothing more
constexpr double PLANE_EPS = 1e-11;

// The face planes of the hull of vert[0 .. nv). Returns their number; < 0 and a message when the
// vertices span no volume. Duplicate and interior vertices are allowed.
inline int hull_planes(const double (*vert)[3], int nv, std::vector<Plane>& out, std::string& err) {
  out.clear();
  double scale = 0;
  for (int i = 0; i < nv; i++)
    for (int k = 0; k < 3; k++) scale = fmax(scale, fabs(vert[i][k]));
  for (int i = 0; i < nv; i++)
    for (int j = i + 1; j < nv; j++)
      for (int k = j + 1; k < nv; k++) {
        double a[3], b[3];
        for (int c = 0; c < 3; c++) { a[c] = vert[j][c] - vert[i][c]; b[c] = vert[k][c] - vert[i][c]; }
        double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        // (collinear or repeated vertices: no plane)
        if (!(len > 1e-9 * scale * scale)) continue;
        for (int c = 0; c < 3; c++) n[c] /= len;
        const double off = n[0] * vert[i][0] + n[1] * vert[i][1] + n[2] * vert[i][2];
        bool below = true, above = true;
        for (int v = 0; v < nv && (below || above); v++) {
          const double s = n[0] * vert[v][0] + n[1] * vert[v][1] + n[2] * vert[v][2] - off;
          if (s > PLANE_EPS) below = false;
          if (s < -PLANE_EPS) above = false;
        }
        if (below == above) {
          if (!below) continue;
          err = "the hull's vertices are coplanar";
          return -1;
        }
        Plane p;
        const double sgn = below ? 1.0 : -1.0;
        for (int c = 0; c < 3; c++) p.n[c] = sgn * n[c];
        p.off = sgn * off;
        bool dup = false;
        for (const Plane& q : out)
          if (p.n[0] * q.n[0] + p.n[1] * q.n[1] + p.n[2] * q.n[2] > 1.0 - 1e-12 && fabs(p.off - q.off) < 10 * PLANE_EPS) {
            dup = true;
            break;
          }
        if (!dup) out.push_back(p);
      }
  if (out.size() < 4) {
    err = "the hull's vertices span no volume";
    return -1;
  }
  return (int)out.size();
}

// The planes of every hull of a model, as the device reads them: plane[(e * HULL_MAXPLANE + i) * 4]
// = (n, off) as fp32 for extra collider e = h * PS_HAND_NXGEOM + i, count[e] of them (0: no hull).
// type / v0 / nv: per extra collider its PS_GEOM_* type and vertex range in vert (NH *
// PS_HAND_HULLVERT vertices, stride floats apart: the device model's fp32 copy, or fp64 x 3).
// Refuses, naming the hull, one with more than HULL_MAXPLANE planes.
template <class T>
inline int build_hull_planes(const int* type, const int* v0, const int* nv, const T* vert, int stride,
                             std::vector<float>& plane, std::vector<int>& count, std::string& err) {
  constexpr int NXT = PS_NHAND * PS_HAND_NXGEOM;
  plane.assign((size_t)NXT * HULL_MAXPLANE * 4, 0.f);
  count.assign(NXT, 0);
  std::vector<Plane> pl;
  for (int e = 0; e < NXT; e++) {
    if (type[e] != PS_GEOM_HULL) continue;
    const std::string who = "hull " + std::to_string(e % PS_HAND_NXGEOM) + " of hand " + std::to_string(e / PS_HAND_NXGEOM);
    if (nv[e] < 4 || nv[e] > PS_HULL_MAXVERT || v0[e] < 0 || v0[e] + nv[e] > PS_NHAND * PS_HAND_HULLVERT) {
      err = who + ": vertex range out of bounds";
      return -1;
    }
    double v[PS_HULL_MAXVERT][3];
    for (int i = 0; i < nv[e]; i++)
      for (int c = 0; c < 3; c++) v[i][c] = (double)vert[(size_t)(v0[e] + i) * stride + c];
    std::string why;
    const int n = hull_planes(v, nv[e], pl, why);
    if (n < 0) {
      err = who + ": " + why;
      return -1;
    }
    if (n > HULL_MAXPLANE) {
      err = who + " has " + std::to_string(n) + " face planes; the ray caster takes at most " +
            std::to_string(HULL_MAXPLANE) + " per hull";
      return -1;
    }
    count[e] = n;
    for (int i = 0; i < n; i++) {
      float* p = &plane[((size_t)e * HULL_MAXPLANE + i) * 4];
      for (int c = 0; c < 3; c++) p[c] = (float)pl[i].n[c];
      p[3] = (float)pl[i].off;
    }
  }
  return 0;
}

}  // namespace psr
