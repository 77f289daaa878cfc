// render.inc - ray-cast cameras over the envs' analytic scene (ps_render, include/pianosim.h).
// Included by pianosim.hip after struct ps_env. Two launches on the caller's stream:
//
//   1. render_scene_kernel, one wave per selected env: its own forward kinematics from the env's
//      qpos row (with the episode's hand-root y shift), every key rotated about its anchor, and a
//      world-space record per object into the handle's scratch: R_NPRIM = 64 colliders + 88 keys +
//      the base records of R_WORDS = 16 floats,
//        capsule  p0 (3), radius, p1 (3)
//        box      centre (3), rotation world <- geom row-major (9), half sizes (3)
//        hull     centre (3), rotation (9), bounding radius, plane count, extra collider index
//      and in word 15 of each: colour index | type << 8 (type 0: not drawn).
//   2. render_rays_kernel, one workgroup of 256 threads per (selected env, 16 x 16 pixel tile):
//      the record into LDS with 16-byte loads, the objects whose bounding sphere touches the tile's
//      four frustum planes into a compact LDS list (in id order: the result does not depend on
//      thread timing), then every thread traces its pixel over that list. All lanes read the same
//      primitive at a time (LDS broadcast), the loop count is wave-uniform.
//
// It reads env memory and the model, and writes the scratch and the caller's images only. The
// fp64 restatement the tests hold it to: tests/render_ref.py.

constexpr int R_NPRIM = NCOLL + NK + 1;  // global collider ids, then 64 + key, then the base
constexpr int R_BASE = NCOLL + NK;       // 152; the floor (153) has no record
constexpr int R_FLOOR = R_BASE + 1;
constexpr int R_WORDS = 16;
constexpr int R_TILE = 16;
constexpr int R_THREADS = R_TILE * R_TILE;
enum : int { RT_NONE = 0, RT_CAPSULE = 1, RT_BOX = 2, RT_HULL = 3 };
static_assert(R_BASE == 152 && R_FLOOR == 153, "the segmentation ids of pianosim.h");

// PS_RENDER_COLOR_* of pianosim.h
__constant__ float r_color[PS_RENDER_NCOLOR][3] = {
    {0.9f, 0.9f, 0.9f}, {0.1f, 0.1f, 0.1f}, {0.15f, 0.15f, 0.15f}, {0.2f, 0.8f, 0.2f},
    {0.8f, 0.2f, 0.8f}, {0.8f, 0.2f, 0.2f}, {0.2f, 0.8f, 0.8f}, {0.2f, 0.2f, 0.8f}, {0.8f, 0.8f, 0.2f},
    {0.6f, 0.6f, 0.6f}, {0.2f, 0.3f, 0.4f}, {0.05f, 0.05f, 0.1f}};

struct RCam {
  float pos[3], x[3], y[3], z[3];  // z = x cross y: the camera looks along -z
  float th;                        // tan(fovy / 2)
};

// --- small fp32 helpers on plain arrays
__device__ __forceinline__ float r_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void r_mv(const float* R, const float* a, float* o) {  // o = R a
  o[0] = R[0] * a[0] + R[1] * a[1] + R[2] * a[2];
  o[1] = R[3] * a[0] + R[4] * a[1] + R[5] * a[2];
  o[2] = R[6] * a[0] + R[7] * a[1] + R[8] * a[2];
}
__device__ __forceinline__ void r_mtv(const float* R, const float* a, float* o) {  // o = R' a
  o[0] = R[0] * a[0] + R[3] * a[1] + R[6] * a[2];
  o[1] = R[1] * a[0] + R[4] * a[1] + R[7] * a[2];
  o[2] = R[2] * a[0] + R[5] * a[1] + R[8] * a[2];
}
__device__ __forceinline__ void r_mm(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Launch 1. rec: [n_sel][R_NPRIM][R_WORDS]. An env index outside [0, n) writes nothing and counts
// in *n_bad (the rays kernel skips it the same way).
__global__ void __launch_bounds__(64) render_scene_kernel(const DevModel* __restrict__ m, const float* __restrict__ qpos,
                                                          const float* __restrict__ hand_dy,
                                                          const int* __restrict__ t_idx, const Song songs, const int hand,
                                                          const int* __restrict__ envs, const int n, const int flags,
                                                          float* __restrict__ rec, int* __restrict__ n_bad) {
  __shared__ float bR[NBT][9], bo[NBT][3];
  const int sel = blockIdx.x, lane = threadIdx.x;
  const int e = envs ? envs[sel] : sel;
  if (e < 0 || e >= n) {
    if (lane == 0 && n_bad) atomicAdd(n_bad, 1);
    return;
  }
  const float* q = qpos + (size_t)e * NV;
  const float dy = hand_dy[e];
  // forward kinematics, one tree level at a time (a body's parent is one level up)
  for (int L = 0; L < m->nlev; L++) {
    for (int idx = m->lev_start[L] + lane; idx < m->lev_start[L + 1]; idx += 64) {
      const int B = m->lev_body[idx], p = m->body_parent[B];
      float R[9], o[3];
      if (p < 0) {
        for (int k = 0; k < 9; k++) R[k] = m->body_Q[B][k];
        for (int k = 0; k < 3; k++) o[k] = m->body_pos[B][k];
        o[1] += dy;
      } else {
        float t[3];
        r_mm(bR[p], m->body_Q[B], R);
        r_mv(bR[p], m->body_pos[B], t);
        for (int k = 0; k < 3; k++) o[k] = bo[p][k] + t[k];
      }
      for (int j = 0; j < m->body_ndof[B]; j++) {
        const int g = m->body_dof[B] + j;
        const float a = q[NK + g];
        const float* ax = m->dof_axis[g];
        if (m->dof_type[g] == 1) {  // slide
          float w[3];
          r_mv(R, ax, w);
          for (int k = 0; k < 3; k++) o[k] += w[k] * a;
        } else {  // hinge: Rodrigues
          float s, c;
          sincosf(a, &s, &c);
          const float C1 = 1.f - c, x = ax[0], y = ax[1], z = ax[2];
          const float A[9] = {c + x * x * C1, x * y * C1 - z * s, x * z * C1 + y * s,
                              y * x * C1 + z * s, c + y * y * C1, y * z * C1 - x * s,
                              z * x * C1 - y * s, z * y * C1 + x * s, c + z * z * C1};
          float T[9];
          r_mm(R, A, T);
          for (int k = 0; k < 9; k++) R[k] = T[k];
        }
      }
      for (int k = 0; k < 9; k++) bR[B][k] = R[k];
      for (int k = 0; k < 3; k++) bo[B][k] = o[k];
    }
    __syncthreads();
  }
  float* out = rec + (size_t)sel * R_NPRIM * R_WORDS;
  // colliders: lane g is global collider g
  {
    float w[R_WORDS];
    for (int k = 0; k < R_WORDS; k++) w[k] = 0.f;
    const int B = m->geom_body[lane];
    int type = RT_NONE, color = PS_RENDER_COLOR_HAND;
    if (flags & PS_RENDER_COLORIZE)
      for (int s = 0; s < NH * PS_NFINGER; s++)
        if (m->site_body[s] == B) color = PS_RENDER_COLOR_FINGER0 + s % PS_NFINGER;
    if (lane < NGT) {
      if (m->geom_r[lane] >= 0.f) {
        type = RT_CAPSULE;
        float c[3], a[3];
        r_mv(bR[B], m->geom_pos[lane], c);
        r_mv(bR[B], m->geom_axis[lane], a);
        const float hl = m->geom_hl[lane];
        for (int k = 0; k < 3; k++) {
          c[k] += bo[B][k];
          w[k] = c[k] - a[k] * hl;
          w[4 + k] = c[k] + a[k] * hl;
        }
        w[3] = m->geom_r[lane];
      }
    } else {
      const int x = lane - NGT;
      if (m->x_type[x] != PS_GEOM_NONE) {
        type = m->x_type[x] == PS_GEOM_BOX ? RT_BOX : RT_HULL;
        float c[3];
        r_mv(bR[B], m->x_pos[x], c);
        for (int k = 0; k < 3; k++) w[k] = c[k] + bo[B][k];
        r_mm(bR[B], m->x_Q[x], w + 3);
        if (type == RT_BOX) {
          for (int k = 0; k < 3; k++) w[12 + k] = m->x_hs[x][k];
        } else {
          w[12] = m->x_rb[x];
          w[14] = __int_as_float(x);  // (the plane count, word 13, is the rays kernel's to look up)
        }
      }
    }
    w[15] = __int_as_float(color | type << 8);
    float4* o4 = reinterpret_cast<float4*>(out + lane * R_WORDS);
    for (int k = 0; k < 4; k++) o4[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  }
  // keys (two rounds of lanes) and the base
  const Song song = song_of(songs, e);
  const int t_goal = t_idx[e] - 1;  // the goal row of the step just played (none after a reset)
  const bool goal_ok = (flags & PS_RENDER_COLORIZE) && t_goal >= 0 && t_goal < song.T;
  const int cnt = goal_ok ? min(song.count[t_goal], PS_MAX_NOTES) : 0;
  for (int k = lane; k <= NK; k += 64) {
    float w[R_WORDS];
    for (int i = 0; i < R_WORDS; i++) w[i] = 0.f;
    int color;
    if (k == NK) {
      for (int i = 0; i < 3; i++) { w[i] = m->base_pos[i]; w[12 + i] = m->base_half[i]; }
      w[3] = w[7] = w[11] = 1.f;
      color = PS_RENDER_COLOR_BASE;
    } else {
      const float a = q[k];
      float s, c;
      sincosf(a, &s, &c);
      const float R[9] = {c, 0.f, s, 0.f, 1.f, 0.f, -s, 0.f, c};  // about +y
      float t[3];
      r_mv(R, m->key_anchor[k], t);
      for (int i = 0; i < 3; i++) {
        w[i] = m->key_pos[k][i] + m->key_anchor[k][i] - t[i];
        w[12 + i] = m->key_half[k][i];
      }
      for (int i = 0; i < 9; i++) w[3 + i] = R[i];
      const int pc = k % 12;  // key 0 is A0: A# C# D# F# G# are black
      color = (pc == 1 || pc == 4 || pc == 6 || pc == 9 || pc == 11) ? PS_RENDER_COLOR_BLACK : PS_RENDER_COLOR_WHITE;
      const float khi = m->key_hi[k];
      const bool act = fabsf(fminf(fmaxf(a, m->key_lo[k]), khi) - khi) <= KEY_THRESHOLD;
      if (act) {
        if (flags & PS_RENDER_ACTIVATION) color = PS_RENDER_COLOR_ACTIVATION;
      } else {
        for (int i = 0; i < cnt; i++) {
          const int f = song.fingers[t_goal * PS_MAX_NOTES + i];
          if (song.keys[t_goal * PS_MAX_NOTES + i] != k || f < 0 || f >= 2 * PS_NFINGER) continue;
          if (hand && (f < PS_NFINGER) != (hand == PS_HAND_RIGHT)) continue;  // the one-hand task: its hand's notes
          color = PS_RENDER_COLOR_FINGER0 + f % PS_NFINGER;
        }
      }
    }
    w[15] = __int_as_float(color | RT_BOX << 8);
    float4* o4 = reinterpret_cast<float4*>(out + (NCOLL + k) * R_WORDS);
    for (int i = 0; i < 4; i++) o4[i] = make_float4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  }
}

// --- intersections: ray o + t d, d not normalised; the first entering hit with t > 0, or none.
// On a hit nearer than `best` they update best and the (unnormalised where noted) normal.

// sphere about c: through the ray's closest point to the centre, which keeps r^2 - |l|^2 free of
// the cancellation of the textbook discriminant
__device__ __forceinline__ void r_sphere(const float* o, const float* d, const float dd, const float* c, const float r,
                                         float& best, float* nrm, bool& hit) {
  const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
  const float tm = -r_dot(oc, d) / dd;
  const float l[3] = {oc[0] + d[0] * tm, oc[1] + d[1] * tm, oc[2] + d[2] * tm};
  const float disc = r * r - r_dot(l, l);
  if (disc < 0.f) return;
  const float t = tm - sqrtf(disc / dd);
  if (t > 0.f && t < best) {
    best = t;
    hit = true;
    for (int k = 0; k < 3; k++) nrm[k] = (oc[k] + d[k] * t) / r;
  }
}

__device__ __forceinline__ void r_capsule(const float* o, const float* d, const float dd, const float* P, float& best,
                                          float* nrm, bool& hit) {
  const float r = P[3];
  float u[3] = {P[4] - P[0], P[5] - P[1], P[6] - P[2]};
  const float len2 = r_dot(u, u);
  r_sphere(o, d, dd, P, r, best, nrm, hit);
  if (len2 < 1e-12f) return;  // p0 == p1: a sphere
  r_sphere(o, d, dd, P + 4, r, best, nrm, hit);
  const float len = sqrtf(len2), il = 1.f / len;
  for (int k = 0; k < 3; k++) u[k] *= il;
  const float oc[3] = {o[0] - P[0], o[1] - P[1], o[2] - P[2]};
  const float du = r_dot(d, u), ou = r_dot(oc, u);
  const float dp[3] = {d[0] - du * u[0], d[1] - du * u[1], d[2] - du * u[2]};
  const float op[3] = {oc[0] - ou * u[0], oc[1] - ou * u[1], oc[2] - ou * u[2]};
  const float A = r_dot(dp, dp);
  if (A < 1e-12f * dd) return;  // along the axis: the end spheres are the whole silhouette
  const float tm = -r_dot(op, dp) / A;
  const float l[3] = {op[0] + dp[0] * tm, op[1] + dp[1] * tm, op[2] + dp[2] * tm};
  const float disc = r * r - r_dot(l, l);
  if (disc < 0.f) return;
  const float t = tm - sqrtf(disc / A);
  const float s = ou + du * t;
  if (t > 0.f && t < best && s >= 0.f && s <= len) {
    best = t;
    hit = true;
    for (int k = 0; k < 3; k++) nrm[k] = (op[k] + dp[k] * t) / r;
  }
}

// oriented box by slabs; a ray parallel to a slab is inside it or misses
__device__ __forceinline__ void r_box(const float* o, const float* d, const float* P, float& best, float* nrm, bool& hit) {
  const float oc[3] = {o[0] - P[0], o[1] - P[1], o[2] - P[2]};
  float ol[3], dl[3];
  r_mtv(P + 3, oc, ol);
  r_mtv(P + 3, d, dl);
  float t0 = -INFINITY, t1 = INFINITY;
  int axis = 0;
  for (int k = 0; k < 3; k++) {
    const float h = P[12 + k];
    if (dl[k] == 0.f) {
      if (fabsf(ol[k]) > h) return;
      continue;
    }
    const float inv = 1.f / dl[k];
    const float ta = (-h - ol[k]) * inv, tb = (h - ol[k]) * inv;
    const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
    if (tn > t0) { t0 = tn; axis = k; }
    t1 = fminf(t1, tf);
  }
  if (t0 > t1 || !(t0 > 0.f) || !(t0 < best)) return;
  best = t0;
  hit = true;
  const float sg = dl[axis] > 0.f ? -1.f : 1.f;  // the entering face looks back along the ray
  for (int k = 0; k < 3; k++) nrm[k] = sg * P[3 + 3 * k + axis];
}

// convex hull: the ray clipped in the geom frame against the face planes n . x <= off
__device__ __forceinline__ void r_hull(const float* o, const float* d, const float* P, const float4* __restrict__ pl,
                                       const int npl, float& best, float* nrm, bool& hit) {
  const float oc[3] = {o[0] - P[0], o[1] - P[1], o[2] - P[2]};
  float ol[3], dl[3];
  r_mtv(P + 3, oc, ol);
  r_mtv(P + 3, d, dl);
  float t0 = -INFINITY, t1 = INFINITY;
  int face = 0;
  bool miss = false;
  for (int i = 0; i < npl; i++) {
    const float4 p = pl[i];
    const float dn = p.x * dl[0] + p.y * dl[1] + p.z * dl[2];
    const float dist = p.x * ol[0] + p.y * ol[1] + p.z * ol[2] - p.w;
    if (dn < 0.f) {
      const float t = -dist / dn;
      if (t > t0) { t0 = t; face = i; }
    } else if (dn > 0.f) {
      t1 = fminf(t1, -dist / dn);
    } else if (dist > 0.f) {
      miss = true;
    }
  }
  if (miss || t0 > t1 || !(t0 > 0.f) || !(t0 < best)) return;
  best = t0;
  hit = true;
  const float4 p = pl[face];
  const float nl[3] = {p.x, p.y, p.z};
  r_mv(P + 3, nl, nrm);
}

// Launch 2. planes [NXT][HULL_MAXPLANE] float4, nplane [NXT]. list_stat (may be null): [0] += the
// tile's list length, [1] += 1 (the diagnostic of PS_RENDER_COUNT_LIST).
__global__ void __launch_bounds__(R_THREADS) render_rays_kernel(const float* __restrict__ rec, const RCam cam,
                                                                const int W, const int H, const int tiles_x,
                                                                const int tiles, const int* __restrict__ envs, const int n,
                                                                const float4* __restrict__ planes,
                                                                const int* __restrict__ nplane, uint8_t* __restrict__ rgb,
                                                                float* __restrict__ depth, int* __restrict__ seg,
                                                                unsigned long long* __restrict__ list_stat) {
  __shared__ float4 s_rec4[R_NPRIM * R_WORDS / 4];
  __shared__ int s_list[R_NPRIM];
  __shared__ int s_wcount[R_THREADS / 64];
  const float* s_rec = reinterpret_cast<const float*>(s_rec4);
  const int tid = threadIdx.x;
  const int sel = blockIdx.x / tiles, tile = blockIdx.x - sel * tiles;
  const int e = envs ? envs[sel] : sel;
  if (e < 0 || e >= n) return;  // (counted by the scene kernel; the image stays as it was)
  const float4* src = reinterpret_cast<const float4*>(rec + (size_t)sel * R_NPRIM * R_WORDS);
  for (int i = tid; i < R_NPRIM * R_WORDS / 4; i += R_THREADS) s_rec4[i] = src[i];
  __syncthreads();
  const int r0 = (tile / tiles_x) * R_TILE, c0 = (tile % tiles_x) * R_TILE;
  const float tw = cam.th * (float)W / (float)H;
  // cull: object tid against the tile's four frustum planes, in camera coordinates (X right, Y up,
  // Z the depth): inside the left plane when X - pxlo Z >= 0, and so on
  bool keep = false;
  if (tid < R_NPRIM) {
    const float* P = s_rec + tid * R_WORDS;
    const int type = __float_as_int(P[15]) >> 8;
    if (type != RT_NONE) {
      float c[3], rad;
      if (type == RT_CAPSULE) {
        const float u[3] = {P[4] - P[0], P[5] - P[1], P[6] - P[2]};
        for (int k = 0; k < 3; k++) c[k] = 0.5f * (P[k] + P[4 + k]);
        rad = 0.5f * sqrtf(r_dot(u, u)) + P[3];
      } else {
        for (int k = 0; k < 3; k++) c[k] = P[k];
        rad = type == RT_BOX ? sqrtf(r_dot(P + 12, P + 12)) : P[12];
      }
      rad = rad * 1.001f + 1e-5f;  // (fp32 rounding of the test itself: keep when in doubt)
      const float v[3] = {c[0] - cam.pos[0], c[1] - cam.pos[1], c[2] - cam.pos[2]};
      const float X = r_dot(v, cam.x), Y = r_dot(v, cam.y), Z = -r_dot(v, cam.z);
      const float pxlo = (2.f * (float)c0 / (float)W - 1.f) * tw, pxhi = (2.f * (float)(c0 + R_TILE) / (float)W - 1.f) * tw;
      const float pyhi = (1.f - 2.f * (float)r0 / (float)H) * cam.th, pylo = (1.f - 2.f * (float)(r0 + R_TILE) / (float)H) * cam.th;
      keep = X - pxlo * Z >= -rad * sqrtf(1.f + pxlo * pxlo) && pxhi * Z - X >= -rad * sqrtf(1.f + pxhi * pxhi) &&
             Y - pylo * Z >= -rad * sqrtf(1.f + pylo * pylo) && pyhi * Z - Y >= -rad * sqrtf(1.f + pyhi * pyhi);
    }
  }
  const unsigned long long mask = __ballot(keep);
  const int wave = tid >> 6, wl = tid & 63;
  if (wl == 0) s_wcount[wave] = __popcll(mask);
  __syncthreads();
  int base = 0, nlist = 0;
  for (int w = 0; w < R_THREADS / 64; w++) {
    if (w < wave) base += s_wcount[w];
    nlist += s_wcount[w];
  }
  if (keep) s_list[base + __popcll(mask & ((1ull << wl) - 1ull))] = tid;
  __syncthreads();
  if (tid == 0 && list_stat) {
    atomicAdd(&list_stat[0], (unsigned long long)nlist);
    atomicAdd(&list_stat[1], 1ull);
  }
  // trace
  const int r = r0 + tid / R_TILE, c = c0 + tid % R_TILE;
  const float py = (1.f - 2.f * ((float)r + 0.5f) / (float)H) * cam.th;
  const float px = (2.f * ((float)c + 0.5f) / (float)W - 1.f) * tw;
  float d[3];
  for (int k = 0; k < 3; k++) d[k] = px * cam.x[k] + py * cam.y[k] - cam.z[k];
  const float dd = r_dot(d, d);
  float best = INFINITY, nrm[3] = {0.f, 0.f, 0.f};
  int id = -1;
  for (int li = 0; li < nlist; li++) {
    const int g = s_list[li];
    const float* P = s_rec + g * R_WORDS;
    const int type = __float_as_int(P[15]) >> 8;
    bool hit = false;
    if (type == RT_CAPSULE) {
      r_capsule(cam.pos, d, dd, P, best, nrm, hit);
    } else if (type == RT_BOX) {
      r_box(cam.pos, d, P, best, nrm, hit);
    } else {
      const int x = __builtin_amdgcn_readfirstlane(__float_as_int(P[14]));
      r_hull(cam.pos, d, P, planes + (size_t)x * psr::HULL_MAXPLANE, __builtin_amdgcn_readfirstlane(nplane[x]), best, nrm, hit);
    }
    if (hit) id = g;
  }
  int color = PS_RENDER_COLOR_BACKGROUND;
  if (id >= 0) color = __float_as_int(s_rec[id * R_WORDS + 15]) & 0xff;
  // the floor: the plane z = 0 from above
  if (d[2] < 0.f && cam.pos[2] > 0.f) {
    const float t = -cam.pos[2] / d[2];
    if (t < best) {
      best = t;
      id = R_FLOOR;
      color = PS_RENDER_COLOR_FLOOR;
      nrm[0] = nrm[1] = 0.f;
      nrm[2] = 1.f;
    }
  }
  if (r >= H || c >= W) return;  // a partial tile's lanes trace with the others and write nothing
  const size_t pix = ((size_t)sel * H + r) * W + c;
  if (depth) depth[pix] = best;
  if (seg) seg[pix] = id;
  if (rgb) {
    float s = 1.f;
    if (id >= 0) s = PS_RENDER_AMBIENT + PS_RENDER_DIFFUSE * fmaxf(0.f, -r_dot(nrm, d) / sqrtf(dd));
    for (int k = 0; k < 3; k++)
      rgb[pix * 3 + k] = (uint8_t)(int)(fminf(fmaxf(r_color[color][k] * s, 0.f), 1.f) * 255.f + 0.5f);
  }
}

// the first ps_render of a handle: the hull face planes (render_build.h) from the device model's
// vertices, and the list counter. Init-time: it allocates and synchronises.
static int render_init(ps_env* E) {
  std::unique_ptr<DevModel> hm(new DevModel);
  HIPCHK(hipMemcpy(hm.get(), E->d_model, sizeof(DevModel), hipMemcpyDeviceToHost));
  std::vector<float> plane;
  std::vector<int> count;
  std::string err;
  if (psr::build_hull_planes(hm->x_type, hm->x_v0, hm->x_nv, &hm->hull_v[0][0], 4, plane, count, err))
    return fail("ps_render: " + err);
  DevMem& mem = E->render_mem;
  hipError_t e = mem.upload(E->r_planes, plane.data(), plane.size());
  if (e == hipSuccess) e = mem.upload(E->r_nplane, count.data(), count.size());
  if (e == hipSuccess) e = mem.alloc(E->r_stat, 2, true);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    mem.clear();
    return fail(std::string("ps_render: ") + hipGetErrorString(e));
  }
  E->r_ready = true;
  return 0;
}

extern "C" {

int ps_render(ps_env* E, const ps_camera* cam, int width, int height, const int32_t* envs, int n_sel, uint32_t flags,
              uint8_t* rgb, float* depth, int32_t* seg, int32_t* n_bad, void* stream) {
  if (!E || !cam) return fail("null argument");
  if (width <= 0 || height <= 0 || n_sel <= 0) return fail("ps_render: width, height and n_sel must be positive");
  if (width > 16384 || height > 16384) return fail("ps_render: an image side over 16384");
  if (!envs && n_sel != E->n) return fail("ps_render: envs == NULL renders all " + std::to_string(E->n) + " envs: n_sel must say so");
  if (!(cam->fovy_deg > 0.0 && cam->fovy_deg < 180.0)) return fail("ps_render: fovy outside (0, 180) degrees");
  if (!rgb && !depth && !seg) return fail("ps_render: rgb, depth and seg are all NULL");
  if (flags & ~(uint32_t)PS_RENDER_ALL) return fail("ps_render: unknown flag bits");
  // x and y orthonormalised (Gram-Schmidt, x first), in fp64
  double x[3], y[3], z[3], nx = 0, ny = 0, xy = 0;
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(cam->pos[k]) || !std::isfinite(cam->x[k]) || !std::isfinite(cam->y[k])) return fail("ps_render: a non-finite camera");
    nx += cam->x[k] * cam->x[k];
  }
  nx = sqrt(nx);
  if (!(nx > 1e-9)) return fail("ps_render: degenerate camera x axis");
  for (int k = 0; k < 3; k++) { x[k] = cam->x[k] / nx; xy += x[k] * cam->y[k]; }
  for (int k = 0; k < 3; k++) { y[k] = cam->y[k] - xy * x[k]; ny += y[k] * y[k]; }
  ny = sqrt(ny);
  double ylen = 0;
  for (int k = 0; k < 3; k++) ylen += cam->y[k] * cam->y[k];
  if (!(ny > 1e-6 * sqrt(ylen)) || !(ny > 1e-9)) return fail("ps_render: degenerate camera y axis (zero, or parallel to x)");
  for (int k = 0; k < 3; k++) y[k] /= ny;
  z[0] = x[1] * y[2] - x[2] * y[1]; z[1] = x[2] * y[0] - x[0] * y[2]; z[2] = x[0] * y[1] - x[1] * y[0];
  RCam rc;
  for (int k = 0; k < 3; k++) { rc.pos[k] = (float)cam->pos[k]; rc.x[k] = (float)x[k]; rc.y[k] = (float)y[k]; rc.z[k] = (float)z[k]; }
  rc.th = (float)tan(0.5 * cam->fovy_deg * M_PI / 180.0);
  const int tiles_x = (width + R_TILE - 1) / R_TILE, tiles_y = (height + R_TILE - 1) / R_TILE;
  const long long groups = (long long)tiles_x * tiles_y * n_sel;
  if (groups > 0x7fffffffLL) return fail("ps_render: more than 2^31 tiles in one call");
  GUARD(E);
  if (!E->r_ready && render_init(E)) return -1;
  if ((size_t)n_sel > E->r_rec_cap) {  // the scene scratch grows to the largest selection so far
    E->render_rec_mem.clear();         // (hipFree waits for the launches that read the old one)
    E->r_rec = nullptr;
    E->r_rec_cap = 0;
    HIPCHK(E->render_rec_mem.alloc(E->r_rec, (size_t)n_sel * R_NPRIM * R_WORDS, false));
    E->r_rec_cap = (size_t)n_sel;
  }
  Song song{E->T, E->d_goal, E->d_count, E->d_keys, E->d_fingers, 0, nullptr};
  if (E->aug_on) song = Song{E->T, E->aug.goal, E->aug.count, E->aug.keys, E->aug.fingers, E->aug.T_cap, E->aug.T};
  hipLaunchKernelGGL(render_scene_kernel, dim3(n_sel), dim3(64), 0, (hipStream_t)stream, E->d_model, E->qpos, E->hand_dy,
                     E->t_idx, song, (int)E->cfg.hand_side, envs, E->n, (int)flags, E->r_rec, n_bad);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(render_rays_kernel, dim3((unsigned)groups), dim3(R_THREADS), 0, (hipStream_t)stream, E->r_rec, rc,
                     width, height, tiles_x, tiles_x * tiles_y, envs, E->n, (const float4*)E->r_planes, E->r_nplane, rgb,
                     depth, seg, (flags & PS_RENDER_COUNT_LIST) ? E->r_stat : nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

int ps_render_list_stats(ps_env* E, uint64_t* sum_tiles, int reset) {
  if (!E || !sum_tiles) return fail("null argument");
  if (!E->r_ready) return fail("ps_render_list_stats: the handle has not rendered");
  GUARD(E);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(sum_tiles, E->r_stat, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(hipMemset(E->r_stat, 0, 2 * sizeof(uint64_t)));
  return 0;
}

}  // extern "C"
