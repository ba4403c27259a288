// Shared device and host code of the ground -> satellite direction (the pose loop and its backward: lm_g2s.hip; the pose score:
// g2s_pose_score.hip): the pixel set-up of both projections, pose -> coefficients, and what the entry points require of a level.
#pragma once
#include "lm_common.h"

#define G2S_COEF_N 24   // a[3] b[3] c[3]  (uv1_k = a_k*v_c + b_k*u_c + c_k)   dx[3] dy[3]   dth_a[3] dth_b[3]   pad[3]

struct __attribute__((aligned(16))) G2sPix {
  int off, dxo, dyo;            // element offsets of the NW tap and the +x / +y neighbours in the ground map
  float wx0, wx1, wy0, wy1;     // clamped-corner bilinear weights x in-bounds mask (jacobian.py:146-177)
  float j0u, j0v, j1u, j1v, j2u, j2v;   // d(uv)/d(shift_u, shift_v, heading) at this pixel (0 where z <= 1e-6)
  float wt;                     // LM weight: projected confidence (or 1)
  float pad0, pad1;
};

// in-plane coefficients (proj == 1): cos, sin, T_u + A/2, T_v + A/2, d(u)/d(shift_u), d(v)/d(shift_v), k = rot*pi/180, A/2
enum { IP_C = 0, IP_S, IP_TU, IP_TV, IP_JU, IP_JV, IP_K, IP_HALF };

struct __attribute__((aligned(16))) G2sIpPix {
  int off, dxo, dyo;
  float wx0, wx1, wy0, wy1;
  float j2u, j2v;               // d(uv)/d(heading) = k dR/dtheta (p - A/2)
  float pad0, pad1, pad2;
};

// (u, v) of satellite pixel (row, col) under the in-plane warp and its heading column (models_kitti.py:303-324)
__device__ __forceinline__ void g2s_ip_uv(const double* cf, int row, int col, double& u, double& v, double& j2u, double& j2v) {
  const double uc = (double)col - cf[IP_HALF], vc = (double)row - cf[IP_HALF];
  const double ru = cf[IP_C] * uc - cf[IP_S] * vc, rv = cf[IP_S] * uc + cf[IP_C] * vc;
  u = ru + cf[IP_TU]; v = rv + cf[IP_TV];
  j2u = -cf[IP_K] * rv; j2v = cf[IP_K] * ru;       // dR/dtheta (uc, vc) = (-s uc - c vc, c uc - s vc) = (-rv, ru)
}

template <int C>
__device__ __forceinline__ G2sIpPix g2s_ip_pixel(const double* cf, int row, int col, int h, int w) {
  double u, v, j2u, j2v;
  g2s_ip_uv(cf, row, col, u, v, j2u, j2v);
  const double limx = (double)(w - 1), limy = (double)(h - 1);
  const bool inb = (u >= 0.0) && (u <= limx) && (v >= 0.0) && (v <= limy);  // jacobian.py:168-170
  G2sIpPix o;
  o.pad0 = o.pad1 = o.pad2 = 0.f;
  if (inb) {
    const double x0 = floor(u), y0 = floor(v);
    const double x1 = fmin(x0 + 1.0, limx), y1 = fmin(y0 + 1.0, limy);
    o.wx0 = (float)(x1 - u); o.wx1 = (float)(u - x0);
    o.wy0 = (float)(y1 - v); o.wy1 = (float)(v - y0);
    const int ix0 = (int)x0, iy0 = (int)y0;
    o.off = (iy0 * w + ix0) * C;
    o.dxo = ((int)x1 - ix0) * C;
    o.dyo = ((int)y1 - iy0) * w * C;
    o.j2u = (float)j2u; o.j2v = (float)j2v;
  } else {
    o.wx0 = o.wx1 = o.wy0 = o.wy1 = 0.f;
    o.off = o.dxo = o.dyo = 0;
    o.j2u = o.j2v = 0.f;
  }
  return o;
}

template <int C, bool USE_W, int PROJ = 0>
__device__ __forceinline__ G2sPix g2s_pixel(const double* cf, int row, int col, int ctr, int h, int w, const float* conf) {
  if constexpr (PROJ == 1) {      // the backward's element loop is shared: the in-plane pixel in the general record
    const G2sIpPix q = g2s_ip_pixel<C>(cf, row, col, h, w);
    const bool inb = (q.wx0 + q.wx1 + q.wy0 + q.wy1) != 0.f;
    G2sPix o;
    o.off = q.off; o.dxo = q.dxo; o.dyo = q.dyo; o.wx0 = q.wx0; o.wx1 = q.wx1; o.wy0 = q.wy0; o.wy1 = q.wy1;
    o.j0u = inb ? (float)cf[IP_JU] : 0.f; o.j0v = 0.f; o.j1u = 0.f; o.j1v = inb ? (float)cf[IP_JV] : 0.f;
    o.j2u = q.j2u; o.j2v = q.j2v; o.wt = 1.f; o.pad0 = o.pad1 = 0.f;
    return o;
  }
  const double vc = (double)(row - ctr), uc = (double)(col - ctr);
  const double q0 = cf[0] * vc + cf[3] * uc + cf[6];
  const double q1 = cf[1] * vc + cf[4] * uc + cf[7];
  const double q2 = cf[2] * vc + cf[5] * uc + cf[8];
  const double z = fmax(q2, 1e-6);                                         // models_kitti.py:121-124
  const bool front = q2 > 1e-6;
  const double iz = 1.0 / z, u = q0 * iz, v = q1 * iz;
  const double limx = (double)(w - 1), limy = (double)(h - 1);
  const bool inb = (u >= 0.0) && (u <= limx) && (v >= 0.0) && (v <= limy);  // jacobian.py:168-170
  G2sPix o;
  o.pad0 = o.pad1 = 0.f;
  if (inb) {
    const double x0 = floor(u), y0 = floor(v);
    const double x1 = fmin(x0 + 1.0, limx), y1 = fmin(y0 + 1.0, limy);
    o.wx0 = (float)(x1 - u); o.wx1 = (float)(u - x0);
    o.wy0 = (float)(y1 - v); o.wy1 = (float)(v - y0);
    const int ix0 = (int)x0, iy0 = (int)y0;
    o.off = (iy0 * w + ix0) * C;
    o.dxo = ((int)x1 - ix0) * C;
    o.dyo = ((int)y1 - iy0) * w * C;
    o.wt = 1.f;
    if (USE_W) {                 // grd_conf_proj = grid_sample(grd_c, uv) (models_kitti.py:298-299)
      const float* cp = conf + (size_t)iy0 * w + ix0;
      const int dx = (int)x1 - ix0, dy = ((int)y1 - iy0) * w;
      o.wt = o.wy0 * (o.wx0 * cp[0] + o.wx1 * cp[dx]) + o.wy1 * (o.wx0 * cp[dy] + o.wx1 * cp[dy + dx]);
    }
    if (front) {                 // duv = d1[0:2]/z - uv1[0:2]*d1[2]/z^2, zero where z <= 1e-6 (143-149)
      const double iz2 = iz * iz;
      const double tx0 = cf[9], tx1 = cf[10], tx2 = cf[11], ty0 = cf[12], ty1 = cf[13], ty2 = cf[14];
      const double tt0 = cf[15] * vc + cf[18] * uc, tt1 = cf[16] * vc + cf[19] * uc, tt2 = cf[17] * vc + cf[20] * uc;
      o.j0u = (float)(tx0 * iz - q0 * tx2 * iz2); o.j0v = (float)(tx1 * iz - q1 * tx2 * iz2);
      o.j1u = (float)(ty0 * iz - q0 * ty2 * iz2); o.j1v = (float)(ty1 * iz - q1 * ty2 * iz2);
      o.j2u = (float)(tt0 * iz - q0 * tt2 * iz2); o.j2v = (float)(tt1 * iz - q1 * tt2 * iz2);
    } else {
      o.j0u = o.j0v = o.j1u = o.j1v = o.j2u = o.j2v = 0.f;
    }
  } else {
    o.wx0 = o.wx1 = o.wy0 = o.wy1 = 0.f;
    o.off = o.dxo = o.dyo = 0;
    o.j0u = o.j0v = o.j1u = o.j1v = o.j2u = o.j2v = 0.f;
    o.wt = USE_W ? 0.f : 1.f;
  }
  return o;
}

// ---------------------------------------------------------------------------------------------
struct G2sGeom { double lat, lon, rot, mpp, sx, sy, half; int proj; };   // sx, sy: intrinsics scale to the level's ground map (111-113)

// proj == 1: pose -> the in-plane coefficients of the level the next step runs on (models_kitti.py:291-302)
__device__ static inline void g2s_ip_coefficients(const G2sGeom& G, double su, double sv, double th, double* cf) {
  const double k = G.rot / 180.0 * 3.14159265358979323846;
  const double ang = th * k;
  cf[IP_C] = cos(ang); cf[IP_S] = sin(ang);
  cf[IP_JU] = -G.lon / G.mpp; cf[IP_JV] = G.lat / G.mpp;
  cf[IP_TU] = cf[IP_JU] * su + G.half; cf[IP_TV] = cf[IP_JV] * sv + G.half;
  cf[IP_K] = k; cf[IP_HALF] = G.half;
  for (int i = IP_HALF + 1; i < G2S_COEF_N; ++i) cf[i] = 0.0;
}

// pose -> the 21 coefficients of the level the next step runs on (models_kitti.py:91-141)
__device__ static inline void g2s_coefficients(const G2sGeom& G, double su, double sv, double th, const float* K9, double* cf) {
  const double k = G.rot / 180.0 * 3.14159265358979323846;
  const double ang = -th * k, c = cos(ang), s = sin(ang);
  double K[3][3];
  for (int j = 0; j < 3; ++j) { K[0][j] = (double)K9[j] * G.sx; K[1][j] = (double)K9[3 + j] * G.sy; K[2][j] = (double)K9[6 + j]; }
  const double T[3] = {sv * G.lat, 1.65, -su * G.lon};                 // utils.get_camera_height() = 1.65
  for (int r = 0; r < 3; ++r) {
    cf[r] = (K[r][0] * c + K[r][2] * s) * G.mpp;                       // P[:,0] = K (c,0,s)'   x X = mpp*v_c
    cf[3 + r] = (-K[r][0] * s + K[r][2] * c) * G.mpp;                  // P[:,2] = K (-s,0,c)'  x Z = mpp*u_c
    cf[6 + r] = K[r][0] * T[0] + K[r][1] * T[1] + K[r][2] * T[2];      // P[:,3] = K T
    cf[9 + r] = -G.lon * K[r][2];                                      // K dT/dx,  dT/dx = lon (0,0,-1)'
    cf[12 + r] = G.lat * K[r][0];                                      // K dT/dy,  dT/dy = lat (1,0,0)'
    cf[15 + r] = k * (K[r][0] * s - K[r][2] * c) * G.mpp;              // K dR[:,0], dR[:,0] = k (s,0,-c)'
    cf[18 + r] = k * (K[r][0] * c + K[r][2] * s) * G.mpp;              // K dR[:,2], dR[:,2] = k (c,0,s)'
  }
  cf[21] = cf[22] = cf[23] = 0.0;
}

// the geometry of level l as the coefficient functions read it
static inline G2sGeom g2s_geom_of(const hla_s2g_config* cfg, const hla_s2g_level& v, int ori_h, int ori_w) {
  G2sGeom g{};
  g.lat = cfg->shift_range_lat; g.lon = cfg->shift_range_lon; g.rot = cfg->rotation_range;
  g.mpp = v.meter_per_pixel; g.proj = cfg->proj; g.half = 0.5 * v.A;      // satmap_sidelength / 2 (304, 309)
  if (!cfg->proj) { g.sx = (double)v.w / ori_w; g.sy = (double)v.h / ori_h; }
  return g;
}

// what every entry point requires of cfg->proj and of the maps it selects (a workspace query has no camera: need_camera = false)
static inline int g2s_validate(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* lv, const float* camera_k, int ori_h,
                               int ori_w, bool need_camera = true) {
  HLA_REQUIRE(cfg->proj == 0 || cfg->proj == 1, "%s: cfg->proj must be 0 (geo) or 1 (in-plane), got %d", who, cfg->proj);
  HLA_REQUIRE(cfg->reach_mode == 0, "%s: cfg->reach_mode belongs to hla_s2g_lm_solve (must be 0 here)", who);
  if (cfg->proj == 0) HLA_REQUIRE(!need_camera || (camera_k && ori_h > 0 && ori_w > 0), "%s: proj 0 needs camera_k and the ground image size", who);
  else HLA_REQUIRE(!cfg->using_weight, "%s: proj 1 has no weighted variant (using_weight must be 0)", who);
  for (int l = 0; l < cfg->n_levels; ++l) {
    const int C = lv[l].C;
    HLA_REQUIRE(C == 256 || C == 128 || C == 64 || (cfg->proj == 1 && C == 16), "%s: unsupported channel count %d", who, C);
    HLA_REQUIRE(lv[l].A > 0 && lv[l].h > 0 && lv[l].w > 0 && lv[l].meter_per_pixel > 0.0, "%s: level %d: bad geometry", who, l);
    HLA_REQUIRE((size_t)lv[l].h * lv[l].w * C < (1u << 31), "%s: ground map too large", who);
    HLA_REQUIRE((size_t)lv[l].A * lv[l].A < (1u << 30), "%s: satellite map too large", who);
  }
  return HLA_OK;
}
