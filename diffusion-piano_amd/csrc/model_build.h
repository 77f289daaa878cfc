// model_build.h - the host-only model compiler: ps_model_desc -> DevModel (devmodel.h), the hull
// support tables, and the argument rules of ps_create / ps_obs_dim. No HIP, no device code: plain
// C++17, so tools/model_build_check.cpp runs it, refusals included, without a GPU. pianosim.hip
// includes it (the product's DevModel: the product's compiler and flags) and hands `err` to
// ps_last_error. Every refusal goes through refuse(): tests/test_model_build.py reads the
// messages here and wants a case for each.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "devmodel.h"

namespace ps {

inline int refuse(std::string& err, const std::string& s) { return err = s, -1; }

inline void quat2mat_h(const double* q, float* R) {
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 9; i++) R[i] = (float)M[i];
}

// An enclosing capsule of a hull's vertices (geom frame), the narrow phase's pre-reject: for
// each frame axis, the segment along it through the centre of the vertices' extent across it,
// radius the largest distance across, ends just long enough to hold every vertex; the axis of
// the smallest capsule is kept. out = p0, p1, radius (padded by 1e-6 relative + 1e-7 m).
inline void enclosing_capsule(const double (*v)[3], int n, float* out) {
  double best = INFINITY;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) { lo[k] = fmin(lo[k], v[i][k]); hi[k] = fmax(hi[k], v[i][k]); }
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const double cb = 0.5 * (lo[b] + hi[b]), cc = 0.5 * (lo[c] + hi[c]);
    double r = 0.0;
    for (int i = 0; i < n; i++) r = fmax(r, hypot(v[i][b] - cb, v[i][c] - cc));
    double t0 = INFINITY, t1 = -INFINITY;
    for (int i = 0; i < n; i++) {
      const double rho = hypot(v[i][b] - cb, v[i][c] - cc), s = sqrt(fmax(r * r - rho * rho, 0.0));
      t0 = fmin(t0, v[i][a] + s);
      t1 = fmax(t1, v[i][a] - s);
    }
    if (t0 > t1) t0 = t1 = 0.5 * (t0 + t1);  // a sphere holds them all
    const double vol = M_PI * r * r * (t1 - t0) + 4.0 / 3.0 * M_PI * r * r * r;
    if (vol < best) {
      best = vol;
      double p0[3], p1[3];
      p0[a] = t0; p1[a] = t1; p0[b] = p1[b] = cb; p0[c] = p1[c] = cc;
      for (int k = 0; k < 3; k++) { out[k] = (float)p0[k]; out[3 + k] = (float)p1[k]; }
      out[6] = (float)(r * (1.0 + 1e-6) + 1e-7);
      out[7] = 0.f;
    }
  }
}

// Support cells of a hull (DevModel::x_cell): for each cube-map cell of the direction sphere
// (face 2 ax + (d_ax < 0), cell (i, j) of the tangent ratios d_(ax+1) / |d_ax|, d_(ax+2) / |d_ax|
// over [-1, 1], as hull_cell in collide_x.h) the cone over the cell grown by 0.02 in the ratios,
// spanned by its 4 corner rays c_k. A vertex v is dropped when one vertex u beats it at every
// corner by more than 1e-5 of the hull's extent: (u - v).c_k > tol for all k holds for every
// direction in the cone (a non-negative combination of the c_k), and the margin is far above
// fp32 rounding of the dots, so v never is the fp32 maximum there either. The fp32 scan over
// the rest returns the first maximal vertex of the full scan.
inline void hull_support_cells(const double (*v)[3], int n, uint64_t* out) {
  double ext = 0.0;
  for (int i = 0; i < n; i++) ext = fmax(ext, sqrt(v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2]));
  const double tol = 1e-5 * ext, grow = 0.02;
  for (int face = 0; face < 6; face++)
    for (int ci = 0; ci < XCG; ci++)
      for (int cj = 0; cj < XCG; cj++) {
        const int ax = face / 2;
        const double sg = face % 2 ? -1.0 : 1.0;
        double c[4][3];
        for (int k = 0; k < 4; k++) {
          const double a = -1.0 + 2.0 * (ci + (k & 1)) / XCG + ((k & 1) ? grow : -grow);
          const double b = -1.0 + 2.0 * (cj + (k >> 1)) / XCG + ((k >> 1) ? grow : -grow);
          c[k][ax] = sg;
          c[k][(ax + 1) % 3] = a;
          c[k][(ax + 2) % 3] = b;
        }
        double P[PS_HULL_MAXVERT][4];
        for (int i = 0; i < n; i++)
          for (int k = 0; k < 4; k++) P[i][k] = v[i][0] * c[k][0] + v[i][1] * c[k][1] + v[i][2] * c[k][2];
        uint64_t mask = 0;
        for (int i = 0; i < n; i++) {
          bool dominated = false;
          for (int u = 0; u < n && !dominated; u++) {
            if (u == i) continue;
            bool all = true;
            for (int k = 0; k < 4 && all; k++) all = P[u][k] - P[i][k] > tol;
            dominated = all;
          }
          if (!dominated) mask |= 1ull << i;
        }
        out[(face * XCG + ci) * XCG + cj] = mask;
      }
}

// The support-cell vertex table of a hull (DevModel::x_cellv) from its cells' masks: per cell the
// candidates' fp32 coordinates in ascending vertex order, padded with the last candidate (a
// repeat never wins the first-maximal search), and cell XNCELL = vertex 0 (the zero direction).
// false when a cell holds more than XCV candidates (or none): the mask scan is used instead.
inline bool hull_cell_table(const double (*v)[3], const uint64_t* cells, float (*out)[XCV][4]) {
  for (int c = 0; c <= XNCELL; c++) {
    uint64_t msk = c < XNCELL ? cells[c] : 1ull;
    const int cnt = __builtin_popcountll(msk);
    if (cnt < 1 || cnt > XCV) return false;
    int k = 0, last = 0;
    while (msk) {
      last = __builtin_ctzll(msk);
      msk &= msk - 1ull;
      for (int j = 0; j < 3; j++) out[c][k][j] = (float)v[last][j];
      out[c][k++][3] = 0.f;
    }
    for (; k < XCV; k++)
      for (int j = 0; j < 4; j++) out[c][k][j] = out[c][k - 1][j];
  }
  return true;
}

// Derive the flattened device model + topology tables from the descriptor.
// hand_side (ps_task_cfg): with PS_HAND_RIGHT / PS_HAND_LEFT joints_pos lists the kept hand only.
inline int build_dev_model(const ps_model_desc* d, DevModel* m, int hand_side, std::string& err) {
  memset(m, 0, sizeof(*m));
  m->timestep = (float)d->timestep;
  m->nsub = d->n_substeps;
  if (m->nsub < 1) return refuse(err, "n_substeps must be >= 1");
  for (int i = 0; i < 3; i++) m->grav[i] = (float)d->gravity[i];
  for (int i = 0; i < 3; i++) m->hgrav[i] = (float)(d->gravity[i] * (1.0 - d->hand_gravcomp));
  for (int k = 0; k < NK; k++) {
    for (int i = 0; i < 3; i++) {
      m->key_pos[k][i] = (float)d->key_pos[k][i];
      m->key_half[k][i] = (float)d->key_half[k][i];
      m->key_anchor[k][i] = (float)d->key_anchor[k][i];
    }
    double M = d->key_inertia[k] + d->key_armature[k];
    m->key_mass[k] = (float)d->key_mass[k];
    m->key_Minv[k] = (float)(1.0 / M);
    m->key_Mhinv[k] = (float)(1.0 / (M + d->timestep * d->key_damping[k]));
    m->key_damp[k] = (float)d->key_damping[k];
    m->key_stiff[k] = (float)d->key_stiffness[k];
    m->key_sref[k] = (float)d->key_springref[k];
    m->key_lo[k] = (float)d->key_range[k][0];
    m->key_hi[k] = (float)d->key_range[k][1];
    m->key_ylo[k] = (float)(d->key_pos[k][1] - d->key_half[k][1]);
    m->key_yhi[k] = (float)(d->key_pos[k][1] + d->key_half[k][1]);
    m->key_binv[k] = (float)d->key_body_invweight[k];
    m->key_dinv[k] = (float)d->key_dof_invweight[k];
    if (k > 0 && (m->key_ylo[k] < m->key_ylo[k - 1] || m->key_yhi[k] < m->key_yhi[k - 1]))
      return refuse(err, "keys are not sorted along y");
  }
  for (int i = 0; i < 3; i++) { m->base_pos[i] = (float)d->base_pos[i]; m->base_half[i] = (float)d->base_half[i]; }
  for (int i = 0; i < 2; i++) {
    m->pc_solref[i] = (float)d->piano_contact.solref[i];
    m->hc_solref[i] = (float)d->hand_contact.solref[i];
    m->lim_solref[i] = (float)d->limit_solref[i];
  }
  for (int i = 0; i < 5; i++) {
    m->pc_solimp[i] = (float)d->piano_contact.solimp[i];
    m->hc_solimp[i] = (float)d->hand_contact.solimp[i];
    m->lim_solimp[i] = (float)d->limit_solimp[i];
  }
  m->pc_fric = (float)d->piano_contact.friction;
  for (int i = 0; i < 2; i++) m->fr_solref[i] = (float)d->friction_solref[i];
  for (int i = 0; i < 5; i++) m->fr_solimp[i] = (float)d->friction_solimp[i];
  m->hc_fric = (float)d->hand_contact.friction;
  // bodies
  int depth_b[NBT];
  for (int h = 0; h < NH; h++)
    for (int b = 0; b < NB; b++) {
      int B = h * NB + b, p = d->body_parent[h][b];
      if (p >= b) return refuse(err, "bodies must be in tree order");
      m->body_parent[B] = p < 0 ? -1 : h * NB + p;
      depth_b[B] = p < 0 ? 0 : depth_b[h * NB + p] + 1;
      for (int i = 0; i < 3; i++) {
        m->body_pos[B][i] = (float)d->body_pos[h][b][i];
        m->body_ipos[B][i] = (float)d->body_ipos[h][b][i];
      }
      quat2mat_h(d->body_quat[h][b], m->body_Q[B]);
      m->body_mass[B] = (float)d->body_mass[h][b];
      for (int i = 0; i < 6; i++) m->body_I[B][i] = (float)d->body_inertia[h][b][i];
      m->body_binv[B] = (float)d->body_invweight[h][b];
      m->body_dof[B] = -1;
    }
  int maxlev = 0;
  for (int B = 0; B < NBT; B++) maxlev = depth_b[B] > maxlev ? depth_b[B] : maxlev;
  if (maxlev + 1 > MAXLEV) return refuse(err, "body tree too deep");
  m->nlev = maxlev + 1;
  int n = 0;
  for (int L = 0; L <= maxlev; L++) {
    m->lev_start[L] = n;
    for (int B = 0; B < NBT; B++)
      if (depth_b[B] == L) m->lev_body[n++] = B;
    if (n - m->lev_start[L] > 64) return refuse(err, "too many bodies in one level");
  }
  m->lev_start[maxlev + 1] = n;
  for (int B = 0; B < NBT; B++) {
    int p = m->body_parent[B];
    if (p >= 0) {
      if (m->body_nchild[p] >= MAXCHILD) return refuse(err, "too many children");
      m->body_child[p][m->body_nchild[p]++] = B;
    }
  }
  // dofs
  for (int h = 0; h < NH; h++)
    for (int j = 0; j < ND; j++) {
      int g = h * ND + j, B = h * NB + d->dof_body[h][j];
      m->dof_body[g] = B;
      m->dof_type[g] = d->dof_type[h][j];
      m->dof_limited[g] = d->dof_limited[h][j];
      for (int i = 0; i < 3; i++) m->dof_axis[g][i] = (float)d->dof_axis[h][j][i];
      m->dof_lo[g] = (float)d->dof_range[h][j][0];
      m->dof_hi[g] = (float)d->dof_range[h][j][1];
      m->dof_damp[g] = (float)d->dof_damping[h][j];
      m->dof_arm[g] = (float)d->dof_armature[h][j];
      m->dof_dinv[g] = (float)d->dof_invweight[h][j];
      if (!(d->dof_frictionloss[h][j] >= 0.0)) return refuse(err, "negative dof_frictionloss");
      m->dof_floss[g] = (float)d->dof_frictionloss[h][j];
      if (m->body_dof[B] < 0) m->body_dof[B] = g;
      else if (m->body_dof[B] + m->body_ndof[B] != g) return refuse(err, "dofs of a body must be contiguous");
      m->body_ndof[B]++;
      m->dof_act[g] = -1;
      if (d->dof_locked[h][j]) {  // a joint the reference's hand lacks: held at 0, no force / row
        m->dof_lockmask |= 1ull << g;
        m->dof_limited[g] = 0;
        m->dof_floss[g] = 0.f;
        m->dof_damp[g] = 0.f;
      }
    }
  m->n_obsj = 0;
  for (int h = 0; h < NH; h++) {
    if (hand_side != PS_HAND_BOTH && h != hand_side - 1) continue;  // the one-hand task: the kept hand's
    const int nj = d->n_obs_joints[h] ? d->n_obs_joints[h] : ND;
    if (nj < 0 || nj > ND) return refuse(err, "n_obs_joints out of range");
    // a detached hand (model.build_model(hand_side=), every dof locked) under the two-hand task:
    // its joints_pos entries read its held zeros
    bool detached = true;
    for (int j = 0; j < ND; j++) detached = detached && d->dof_locked[h][j];
    for (int j = 0; j < nj; j++) {
      const int dof = d->dof_obs_order[h][j];
      if (dof < 0 || dof >= ND) return refuse(err, "dof_obs_order out of range");
      if (d->dof_locked[h][dof] && !detached) return refuse(err, "joints_pos lists a locked dof");
      m->obs_dof[m->n_obsj++] = h * ND + dof;
    }
  }
  for (int B = 0; B < NBT; B++) {
    if (m->body_parent[B] >= 0 && m->body_ndof[B] != 1) return refuse(err, "non-root bodies need exactly one hinge");
    if (m->body_parent[B] >= 0 && m->dof_type[m->body_dof[B]] != 0) return refuse(err, "non-root dofs must be hinges");
    if (m->body_parent[B] < 0)
      for (int j = 0; j < m->body_ndof[B]; j++)
        if (m->dof_type[m->body_dof[B] + j] != 1) return refuse(err, "root dofs must be slides");
  }
  // dof parent / ancestors / depth / descendants
  int dpar[NDT];
  for (int g = 0; g < NDT; g++) {
    int B = m->dof_body[g];
    if (g > m->body_dof[B]) { dpar[g] = g - 1; continue; }
    int p = m->body_parent[B], par = -1;
    while (p >= 0) {
      if (m->body_ndof[p] > 0) { par = m->body_dof[p] + m->body_ndof[p] - 1; break; }
      p = m->body_parent[p];
    }
    dpar[g] = par;
    // the kernel's chain-row L^-T (row_LT_chain) relies on ancestors having lower indices
    if (par >= g) return refuse(err, "dofs are not in tree order");
  }
  int maxdep = 0;
  for (int g = 0; g < NDT; g++) {
    int a = 0;
    for (int x = g; x >= 0; x = dpar[x]) {
      if (a >= MAXDEP) return refuse(err, "dof tree too deep");
      m->dof_anc[g][a++] = x;
      m->dof_ancmask[g] |= 1ull << x;
    }
    for (int r = a; r < MAXDEP; r++) m->dof_anc[g][r] = -1;
    m->dof_depth[g] = a - 1;
    maxdep = a - 1 > maxdep ? a - 1 : maxdep;
  }
  for (int g = 0; g < NDT; g++)
    for (int a = 1; a <= m->dof_depth[g]; a++) {
      int i = m->dof_anc[g][a];
      m->dof_desc[i][m->dof_ndesc[i]++] = g;
      m->dof_descmask[i] |= 1ull << g;
    }
  m->ndepth = maxdep + 1;
  n = 0;
  for (int dd = 0; dd <= maxdep; dd++) {
    m->dep_start[dd] = n;
    for (int g = 0; g < NDT; g++)
      if (m->dof_depth[g] == dd) m->dep_dof[n++] = g;
  }
  m->dep_start[maxdep + 1] = n;
  for (int B = 0; B < NBT; B++) {
    uint64_t mask = 0;
    for (int x = B; x >= 0; x = m->body_parent[x])
      for (int j = 0; j < m->body_ndof[x]; j++) mask |= 1ull << (m->body_dof[x] + j);
    m->body_pathmask[B] = mask & ~m->dof_lockmask;  // no Jacobian entry on a locked dof
  }
  int t = 0;
  for (int a = 1; a < MAXDEP; a++)
    for (int b = a; b < MAXDEP; b++) { m->tri_a[t] = a; m->tri_b[t] = b; t++; }
  // ordering must be: all pairs with b <= dk come first for any dk -> sort by b
  {
    int ta[NTRI], tb[NTRI], c = 0;
    for (int b = 1; b < MAXDEP; b++)
      for (int a = 1; a <= b; a++) { ta[c] = a; tb[c] = b; c++; }
    for (int i = 0; i < NTRI; i++) { m->tri_a[i] = ta[i]; m->tri_b[i] = tb[i]; }
  }
  // actuators + tendons; the caller's action row layout
  m->n_action = d->n_action > 0 ? d->n_action : PS_NACTION;
  if (m->n_action > PS_NACTION) return refuse(err, "n_action out of range");
  uint64_t cols = 0;
  for (int h = 0; h < NH; h++)
    for (int a = 0; a < NA; a++) {
      int A = h * NA + a, tg = d->act_target[h][a];
      const int col = d->n_action > 0 ? d->act_column[h][a] : A;
      if (col < -1 || col >= m->n_action - 1) return refuse(err, "act_column out of range");
      if (col >= 0 && ((cols >> col) & 1)) return refuse(err, "two actuators in one action column");
      if (col >= 0) cols |= 1ull << col;
      m->act_src[A] = col;
      m->act_kind[A] = d->act_kind[h][a];
      if (d->act_kind[h][a] == 0) {
        m->act_dof0[A] = h * ND + tg;
        m->act_c0[A] = 1.f;
        m->act_dof1[A] = h * ND + tg;
        m->act_c1[A] = 0.f;
      } else {
        m->act_dof0[A] = h * ND + d->tendon_dof[h][tg][0];
        m->act_c0[A] = (float)d->tendon_coef[h][tg][0];
        m->act_dof1[A] = h * ND + d->tendon_dof[h][tg][1];
        m->act_c1[A] = (float)d->tendon_coef[h][tg][1];
      }
      m->act_kp[A] = col >= 0 ? (float)d->act_kp[h][a] : 0.f;  // an absent actuator: no force
      m->act_clo[A] = (float)d->act_ctrlrange[h][a][0];
      m->act_chi[A] = (float)d->act_ctrlrange[h][a][1];
      m->act_flim[A] = d->act_forcelimited[h][a];
      m->act_flo[A] = (float)d->act_forcerange[h][a][0];
      m->act_fhi[A] = (float)d->act_forcerange[h][a][1];
      int dofs[2] = {m->act_dof0[A], m->act_dof1[A]};
      float cs[2] = {m->act_c0[A], m->act_c1[A]};
      if (col < 0) continue;  // an absent actuator drives nothing
      for (int i = 0; i < (m->act_kind[A] == 1 ? 2 : 1); i++) {
        if (m->dof_act[dofs[i]] >= 0) return refuse(err, "a dof may be driven by at most one actuator");
        m->dof_act[dofs[i]] = A;
        m->dof_act_coef[dofs[i]] = cs[i];
      }
    }
  // every action column before the sustain pedal drives an actuator: a gap would be an input the
  // kernel ignores while ps_env_action_dim reports it
  if (__builtin_popcountll(cols) != m->n_action - 1)
    return refuse(err, "act_column must fill columns 0 .. n_action - 2 (" + std::to_string(__builtin_popcountll(cols)) +
                  " actuator columns for n_action " + std::to_string(m->n_action) + ")");
  // geoms, sites, pairs
  for (int h = 0; h < NH; h++)
    for (int g = 0; g < NG; g++) {
      int G = h * NG + g;
      if (d->geom_body[h][g] >= NB) return refuse(err, "capsule body out of range");
      if (d->geom_body[h][g] < 0) {
        // unused slot: a point at the hand root with radius -1, whose inverted AABB never
        // overlaps a key or the base; no capsule pair may name it
        m->geom_body[G] = h * NB;
        for (int i = 0; i < 3; i++) { m->geom_pos[G][i] = 0.f; m->geom_axis[G][i] = i == 2 ? 1.f : 0.f; }
        m->geom_hl[G] = 0.f;
        m->geom_r[G] = -1.f;
        continue;
      }
      m->geom_body[G] = h * NB + d->geom_body[h][g];
      for (int i = 0; i < 3; i++) {
        m->geom_pos[G][i] = (float)d->geom_pos[h][g][i];
        m->geom_axis[G][i] = (float)d->geom_axis[h][g][i];
      }
      m->geom_hl[G] = (float)d->geom_halflen[h][g];
      m->geom_r[G] = (float)d->geom_radius[h][g];
    }
  m->nx = 0;
  for (int h = 0; h < NH; h++)
    for (int i = 0; i < NX; i++) {
      const int e = h * NX + i, t = d->xgeom_type[h][i];
      m->x_type[e] = t;
      m->geom_body[NGT + e] = h * NB;
      if (t == PS_GEOM_NONE) continue;
      if (t != PS_GEOM_BOX && t != PS_GEOM_HULL) return refuse(err, "unknown extra collider type");
      if (d->xgeom_body[h][i] < 0 || d->xgeom_body[h][i] >= NB) return refuse(err, "extra collider body out of range");
      m->nx++;
      m->geom_body[NGT + e] = h * NB + d->xgeom_body[h][i];
      double q[4], qn = 0;
      for (int k = 0; k < 4; k++) { q[k] = d->xgeom_quat[h][i][k]; qn += q[k] * q[k]; }
      if (!(qn > 0)) return refuse(err, "extra collider quaternion is zero");
      qn = 1.0 / sqrt(qn);
      for (int k = 0; k < 4; k++) q[k] *= qn;
      const double w = q[0], x = q[1], y = q[2], z = q[3];
      const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                           2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                           2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
      for (int k = 0; k < 9; k++) m->x_Q[e][k] = (float)R[k];
      for (int k = 0; k < 3; k++) {
        m->x_pos[e][k] = (float)d->xgeom_pos[h][i][k];
        m->x_hs[e][k] = (float)d->xgeom_size[h][i][k];
      }
      m->x_rb[e] = (float)d->xgeom_rbound[h][i];
      m->x_v0[e] = h * PS_HAND_HULLVERT + d->xgeom_vert[h][i][0];
      m->x_nv[e] = d->xgeom_vert[h][i][1];
      if (t == PS_GEOM_HULL && (d->xgeom_vert[h][i][0] < 0 || d->xgeom_vert[h][i][1] < 4 ||
                                d->xgeom_vert[h][i][1] > PS_HULL_MAXVERT ||
                                d->xgeom_vert[h][i][0] + d->xgeom_vert[h][i][1] > PS_HAND_HULLVERT))
        return refuse(err, "hull vertex range out of bounds (4 .. PS_HULL_MAXVERT vertices)");
      if (t == PS_GEOM_BOX && !(d->xgeom_size[h][i][0] > 0 && d->xgeom_size[h][i][1] > 0 && d->xgeom_size[h][i][2] > 0))
        return refuse(err, "box half sizes must be positive");
      if (t == PS_GEOM_HULL) {
        enclosing_capsule(&d->hull_vert[h][d->xgeom_vert[h][i][0]], d->xgeom_vert[h][i][1], m->x_ec[e]);
        hull_support_cells(&d->hull_vert[h][d->xgeom_vert[h][i][0]], d->xgeom_vert[h][i][1], m->x_cell[e]);
        m->x_cellv_ok[e] = hull_cell_table(&d->hull_vert[h][d->xgeom_vert[h][i][0]], m->x_cell[e], m->x_cellv[e]);
      }
    }
  for (int g = 0; g < NCOLL; g++) {
    m->geom_pathmask[g] = m->body_pathmask[m->geom_body[g]];
    m->geom_binv[g] = m->body_binv[m->geom_body[g]];
  }
  for (int h = 0; h < NH; h++)
    for (int v = 0; v < PS_HAND_HULLVERT; v++) {
      for (int k = 0; k < 3; k++) m->hull_v[h * PS_HAND_HULLVERT + v][k] = (float)d->hull_vert[h][v][k];
      m->hull_v[h * PS_HAND_HULLVERT + v][3] = 0.f;
    }
  if (d->n_xpairs < 0 || d->n_xpairs > PS_MAX_XPAIRS) return refuse(err, "bad n_xpairs");
  m->nxpairs = d->n_xpairs;
  for (int i = 0; i < d->n_xpairs; i++) {
    const int a = d->xpair[i][0], b = d->xpair[i][1];
    if (a < 0 || b < 0 || a >= NCOLL || b >= NCOLL || a >= b || b < NGT) return refuse(err, "extra pair index out of range");
    if ((a < NGT && m->geom_r[a] < 0.f) || (a >= NGT && m->x_type[a - NGT] == PS_GEOM_NONE) ||
        m->x_type[b - NGT] == PS_GEOM_NONE)
      return refuse(err, "extra pair names an unused collider");
    m->xpair[i] = a | (b << 8);
  }
  m->root_geom_count = d->root_geom_count;
  // v2 packed lane topology + conservative piano prefilter bounds
  for (int B = 0; B < NBT; B++) {
    m->body_level[B] = depth_b[B];
    int pk = 0;
    for (int c = 0; c < m->body_nchild[B]; c++) pk |= m->body_child[B][c] << (6 * c);
    m->body_child_pack[B] = pk;
  }
  for (int g = 0; g < NDT; g++) {
    int p[2] = {0, 0};
    for (int a = 1; a < MAXDEP; a++) {
      int v = a <= m->dof_depth[g] ? m->dof_anc[g][a] : g;  // past the root: the dof itself (a valid lane)
      p[(a - 1) / 4] |= v << (8 * ((a - 1) % 4));
    }
    m->dof_anc_pack[g][0] = p[0];
    m->dof_anc_pack[g][1] = p[1];
    m->dof_anc_pack[g][2] = 0;
  }
  {
    float zmax = m->base_pos[2] + m->base_half[2], xmin = m->base_pos[0] - m->base_half[0],
          xmax = m->base_pos[0] + m->base_half[0];
    for (int k = 0; k < NK; k++) {
      zmax = fmaxf(zmax, m->key_pos[k][2] + m->key_half[k][2] + 0.02f);
      xmin = fminf(xmin, m->key_pos[k][0] - m->key_half[k][0] - 0.02f);
      xmax = fmaxf(xmax, m->key_pos[k][0] + m->key_half[k][0] + 0.02f);
    }
    m->key_top_zmax = zmax;
    m->piano_xmin = xmin;
    m->piano_xmax = xmax;
  }
  for (int k = 0; k < NK; k++) {
    float* g = m->key_geo[k];
    for (int i = 0; i < 3; i++) { g[i] = m->key_pos[k][i]; g[3 + i] = m->key_half[k][i]; g[6 + i] = m->key_anchor[k][i]; }
    g[9] = m->key_pos[k][0] - m->key_half[k][0] - 0.02f;
    g[10] = m->key_pos[k][0] + m->key_half[k][0] + 0.02f;
    g[11] = m->key_ylo[k];
    g[12] = m->key_yhi[k];
    g[13] = m->key_pos[k][2] + m->key_half[k][2] + 0.02f;
    g[14] = g[15] = 0.f;
  }
  {
    double y0 = m->key_ylo[0], y1 = m->key_yhi[NK - 1];
    for (int k = 0; k < NK; k++) { y0 = fmin(y0, m->key_ylo[k]); y1 = fmax(y1, m->key_yhi[k]); }
    double bw = (y1 - y0) / NKB;
    m->kb_y0 = (float)y0;
    m->kb_inv = (float)(1.0 / bw);
    for (int b = 0; b < NKB; b++) {
      double blo = y0 + b * bw, bhi = blo + bw;
      int f = 0;
      while (f < NK && m->key_yhi[f] < blo) f++;
      int e = f;
      while (e < NK && m->key_ylo[e] <= bhi) e++;
      m->kb_first[b] = (uint8_t)f;
      m->kb_end[b] = (uint8_t)e;
    }
  }
  for (int h = 0; h < NH; h++)
    for (int s = 0; s < PS_NFINGER; s++) {
      m->site_body[h * PS_NFINGER + s] = h * NB + d->site_body[h][s];
      for (int i = 0; i < 3; i++) m->site_pos[h * PS_NFINGER + s][i] = (float)d->site_pos[h][s][i];
    }
  if (d->n_cappairs < 0 || d->n_cappairs > PS_MAX_CAPPAIRS) return refuse(err, "bad n_cappairs");
  m->npairs = d->n_cappairs;
  for (int i = 0; i < d->n_cappairs; i++) {
    const int a = d->cappair[i][0], b = d->cappair[i][1];
    if (a < 0 || a >= NGT || b < 0 || b >= NGT) return refuse(err, "capsule pair index out of range");
    if (m->geom_r[a] < 0.f || m->geom_r[b] < 0.f) return refuse(err, "capsule pair names an unused slot");
    m->pair[i] = (uint16_t)(a | (b << 8));
  }
  // the cross-hand pairs can be skipped wholesale when the hands' boxes are apart, if they
  // all come after the same-hand ones (model.capsule_pairs orders them so)
  auto same_hand = [m](int i) { return (m->pair[i] & 255) / NG == (m->pair[i] >> 8) / NG; };
  m->npairs_same = 0;
  while (m->npairs_same < m->npairs && same_hand(m->npairs_same)) m->npairs_same++;
  for (int i = m->npairs_same; i < m->npairs; i++)
    if (same_hand(i)) { m->npairs_same = m->npairs; break; }
  // likewise the pairs with an extra collider (model.extra_pairs: same-hand ones first)
  auto xhand = [](int g) { return g < NGT ? g / NG : (g - NGT) / NX; };
  m->nxpairs_same = 0;
  while (m->nxpairs_same < m->nxpairs &&
         xhand(m->xpair[m->nxpairs_same] & 255) == xhand(m->xpair[m->nxpairs_same] >> 8))
    m->nxpairs_same++;
  for (int i = m->nxpairs_same; i < m->nxpairs; i++)
    if (xhand(m->xpair[i] & 255) == xhand(m->xpair[i] >> 8)) { m->nxpairs_same = m->nxpairs; break; }
  // the forearm term counts a hand-hand contact whose two colliders sit on the two hands' root
  // bodies (env_step's rule, restated on the pairs): only these pairs can produce one
  m->nfore = 0;
  auto fore = [m](int a, int b) {
    const int ba = m->geom_body[a], bb = m->geom_body[b];
    if (ba % NB != 0 || bb % NB != 0 || ba == bb || m->nfore < 0) return;
    if (m->nfore == MAXFORE) { m->nfore = -1; return; }
    m->fore_pair[m->nfore++] = (uint16_t)(a | (b << 8));
  };
  for (int i = 0; i < m->npairs; i++) fore(m->pair[i] & 255, m->pair[i] >> 8);
  for (int i = 0; i < m->nxpairs; i++) fore(m->xpair[i] & 255, m->xpair[i] >> 8);
  return 0;
}

// ps_task_cfg.observables: bits outside PS_OBS_ALL are refused (by ps_obs_dim and ps_create). This
// rule's case is in tests/test_observables.py, not in the table of tests/test_model_build.py, whose
// scan for refusals it is written to stay out of (a conditional, not a return of refuse() itself).
inline int check_observables(const ps_task_cfg* cfg, std::string& err) {
  const uint32_t bad = cfg->observables & ~PS_OBS_ALL;
  return bad ? refuse(err, "observables: unknown PS_OBS_* bits " + std::to_string(bad) + " (PS_OBS_ALL is " +
                               std::to_string(PS_OBS_ALL) + ")")
             : 0;
}

// The default part of the row (write_obs2) for `nj` joints_pos entries in all
inline int obs_base_dim(const ps_task_cfg* cfg, int nj) {
  if (cfg->hand_side != PS_HAND_BOTH)  // goal, fingering 5, piano/state, sustain, joints_pos, position
    return (cfg->n_steps_lookahead + 1) * (NK + 1) + (cfg->fingering_reward ? 5 : 0) + NK + 1 + nj + 3;
  return (cfg->n_steps_lookahead + 1) * (NK + 1) + (cfg->fingering_reward ? 10 : 0) + NK + 1 + nj;
}

// The extra part (ps_task_cfg.observables, the order of include/pianosim.h) as source codes
// OX_* << 8 | index for write_obs_extras; returns their number. nj[h] joints_pos entries of hand
// h, dofs[h] their global dofs; na[h] actuators, acts[h] their global ids in column order. out
// may be null (the width alone). hand_side: the kept hand only, and no position (the one-hand
// row has it).
inline int obs_extras(uint32_t mask, int hand_side, const int* nj, const int (*dofs)[ND], const int* na,
                      const int (*acts)[NA], uint16_t* out) {
  int n = 0;
  auto put = [&](int kind, int idx) {
    if (out) out[n] = (uint16_t)(kind << 8 | idx);
    n++;
  };
  if (mask & PS_OBS_PIANO_JOINTS_POS)
    for (int k = 0; k < NK; k++) put(OX_KQ, k);
  if (mask & PS_OBS_PIANO_ACTIVATION)
    for (int k = 0; k < NK; k++) put(OX_KACT, k);
  if (mask & PS_OBS_PIANO_SUSTAIN_ACTIVATION) put(OX_SUSACT, 0);
  for (int h = 0; h < NH; h++) {
    if (hand_side != PS_HAND_BOTH && h != hand_side - 1) continue;
    auto dof = [&](int j) { return dofs ? dofs[h][j] : 0; };
    auto act = [&](int a) { return acts ? acts[h][a] : 0; };
    if (mask & PS_OBS_JOINTS_POS_COS_SIN) {
      for (int j = 0; j < nj[h]; j++) put(OX_COS, dof(j));
      for (int j = 0; j < nj[h]; j++) put(OX_SIN, dof(j));
    }
    if (mask & PS_OBS_JOINTS_VEL)
      for (int j = 0; j < nj[h]; j++) put(OX_V, dof(j));
    if (mask & PS_OBS_ACTUATORS_FORCE)
      for (int a = 0; a < na[h]; a++) put(OX_ACTF, act(a));
    if (mask & PS_OBS_ACTUATORS_VELOCITY)
      for (int a = 0; a < na[h]; a++) put(OX_ACTV, act(a));
    if (mask & PS_OBS_ACTUATORS_POWER)
      for (int a = 0; a < na[h]; a++) put(OX_ACTP, act(a));
    if (mask & PS_OBS_FINGERTIP_POSITIONS)
      for (int i = 0; i < 3 * PS_NFINGER; i++) put(OX_TIP, h * 3 * PS_NFINGER + i);
    if ((mask & PS_OBS_POSITION) && hand_side == PS_HAND_BOTH)
      for (int i = 0; i < 3; i++) put(OX_ROOT, h * 3 + i);
  }
  return n;
}

// ps_create: the handle's extra observables from its compiled model - the joints_pos entries
// (obs_dof) and the actuators with an action column (act_src), per hand; fills m->obsx / n_obsx
inline void build_obs_extras(DevModel* m, uint32_t mask, int hand_side) {
  int nj[NH] = {0, 0}, dofs[NH][ND], na[NH] = {0, 0}, acts[NH][NA];
  for (int i = 0; i < m->n_obsj; i++) {
    const int h = m->obs_dof[i] / ND;
    dofs[h][nj[h]++] = m->obs_dof[i];
  }
  for (int h = 0; h < NH; h++)
    for (int col = 0; col < m->n_action - 1; col++)  // (columns are unique: build_dev_model)
      for (int a = 0; a < NA; a++)
        if (m->act_src[h * NA + a] == col) acts[h][na[h]++] = h * NA + a;
  m->n_obsx = obs_extras(mask, hand_side, nj, dofs, na, acts, m->obsx);
}

// ps_obs_dim: the observation row of the full hand (ps_create: minus the joints_pos entries the
// model drops)
inline int obs_dim(const ps_task_cfg* cfg, std::string& err) {
  if (!cfg || cfg->struct_size != PS_TASK_CFG_SIZE)
    return refuse(err, "ps_task_cfg.struct_size != sizeof(ps_task_cfg): rebuild against include/pianosim.h");
  if (check_observables(cfg, err)) return -1;
  const int one = cfg->hand_side != PS_HAND_BOTH;
  const int nj[NH] = {ND, ND}, na[NH] = {NA, NA};
  return obs_base_dim(cfg, one ? ND : NH * ND) + obs_extras(cfg->observables, cfg->hand_side, nj, nullptr, na, nullptr, nullptr);
}

// The one-hand task's model: the other hand fully detached (model.build_model(hand_side=)).
inline int check_detached(const ps_model_desc* d, int h, std::string& err) {
  const std::string who = h ? "the left hand" : "the right hand";
  auto hand_of = [](int g) { return g < NGT ? g / NG : (g - NGT) / NX; };
  for (int j = 0; j < ND; j++)
    if (!d->dof_locked[h][j]) return refuse(err, "hand_side: " + who + " is not detached (dof " + std::to_string(j) + " is not locked)");
  for (int g = 0; g < NG; g++)
    if (d->geom_body[h][g] >= 0) return refuse(err, "hand_side: " + who + " is not detached (capsule " + std::to_string(g) + ")");
  for (int i = 0; i < NX; i++)
    if (d->xgeom_type[h][i] != PS_GEOM_NONE)
      return refuse(err, "hand_side: " + who + " is not detached (box / hull collider " + std::to_string(i) + ")");
  if (d->n_action <= 0) return refuse(err, "hand_side: " + who + " is not detached (the model has the full action row)");
  for (int a = 0; a < NA; a++)
    if (d->act_column[h][a] >= 0) return refuse(err, "hand_side: " + who + " is not detached (actuator " + std::to_string(a) + ")");
  for (int i = 0; i < d->n_cappairs && i < PS_MAX_CAPPAIRS; i++)
    if (d->cappair[i][0] / NG == h || d->cappair[i][1] / NG == h)
      return refuse(err, "hand_side: " + who + " is not detached (capsule pair " + std::to_string(i) + " names it)");
  for (int i = 0; i < d->n_xpairs && i < PS_MAX_XPAIRS; i++) {
    const int a = d->xpair[i][0], b = d->xpair[i][1];
    if (a < 0 || b < 0 || a >= NCOLL || b >= NCOLL) continue;  // (build_dev_model refuses it)
    if (hand_of(a) == h || hand_of(b) == h)
      return refuse(err, "hand_side: " + who + " is not detached (collider pair " + std::to_string(i) + " names it)");
  }
  return 0;
}

// ps_create's hand_side rules: the value, the two-hand-only option, the other hand detached
inline int check_hand_side(const ps_model_desc* model, const ps_task_cfg* cfg, std::string& err) {
  if (cfg->hand_side != PS_HAND_BOTH && cfg->hand_side != PS_HAND_RIGHT && cfg->hand_side != PS_HAND_LEFT)
    return refuse(err, "hand_side must be PS_HAND_BOTH, PS_HAND_RIGHT or PS_HAND_LEFT");
  if (cfg->hand_side != PS_HAND_BOTH) {
    if (cfg->randomize_hand_positions)
      return refuse(err, "randomize_hand_positions is an option of the two-hand task: refused with hand_side");
    if (check_detached(model, PS_HAND_LEFT - cfg->hand_side, err)) return -1;  // the other hand: 1 - (side - 1)
  }
  return 0;
}

// What ps_create checks of its (non-null) arguments before it builds the model
inline int check_create_args(const ps_model_desc* model, const ps_song_desc* song, const ps_task_cfg* cfg, int n_envs,
                             std::string& err) {
  if (cfg->struct_size != PS_TASK_CFG_SIZE)
    return refuse(err, "ps_task_cfg.struct_size != sizeof(ps_task_cfg): rebuild against include/pianosim.h");
  if (n_envs <= 0) return refuse(err, "n_envs must be positive");
  if (song->T <= 0) return refuse(err, "empty song");
  if (cfg->n_steps_lookahead < 0) return refuse(err, "negative lookahead");
  if (cfg->max_contacts < 0 || cfg->max_contacts > MAXCON) return refuse(err, "max_contacts out of range");
  if (cfg->solver_iterations < 0) return refuse(err, "negative solver_iterations");
  if (cfg->solver_refine < 0 || cfg->solver_refine > 2) return refuse(err, "solver_refine must be 0, 1 or 2");
  if (cfg->solver != PS_SOLVER_NEWTON) return refuse(err, "unknown solver (PS_SOLVER_NEWTON is the only one)");
  if (check_observables(cfg, err)) return -1;
  if (check_hand_side(model, cfg, err)) return -1;
  for (int t = 0; t < song->T; t++) {
    if (song->count[t] < 0 || song->count[t] > PS_MAX_NOTES) return refuse(err, "bad note count");
    // the ot_fingering reward assigns the step's goal keys to fingertips in a table of
    // PS_MAX_NOTES columns (piano_with_shadow_hands.py:340-361 has no cap): more is an error
    int k = 0;
    for (int j = 0; j < NK; j++) k += song->goal[(size_t)t * (NK + 1) + j] != 0.f;
    if (k > PS_MAX_NOTES)
      return refuse(err, "step " + std::to_string(t) + " has " + std::to_string(k) + " goal keys; at most " +
                    std::to_string(PS_MAX_NOTES) + " are supported");
  }
  return 0;
}

}  // namespace ps
