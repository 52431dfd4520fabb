// Rasteriser of posed triangle meshes: every instance's mesh, posed and projected into the frame the instance is seen in,
// z-buffered per pixel -> instance labels, a depth image, the winning face, a visibility class per pixel against an observed
// depth and, on request, the model-space point under every pixel (for a NOCS-normalised model: its NOCS map minus the 0.5
// offset).  The key image (here bits(z) << 32 | posed face), its tie rule, the classes, the projection, the box walk, the
// clear kernel (which zeroes `culled` too) and the common part of the resolve are the z-buffer core's (catre_zbuf.h), shared
// with the splat render; this header holds what is the rasteriser's own.
//
// k_mesh_project   one thread per posed vertex (instance-major): R (s * x) + t with nn_load_point, zbuf_project (the splat's
//                  projection: one function), snapped to 8 fractional bits -> record (xi, yi, bits(z), ok).  From here on
//                  everything is a function of the records alone.
// k_mesh_raster    one LANE sets up one posed face (indices checked, records read, oriented to a positive doubled area, bounding
//                  box clamped to the image).  Faces whose box holds at most MESH_LANE_PX samples are then drawn by their own
//                  lanes side by side (a fine mesh: a face is about a pixel, and a wave that walked them one by one would
//                  leave 60 lanes idle); the WAVE walks the other live faces one after the other with all 64 lanes spread
//                  over the pixels of the face's box (zbuf_each_live, zbuf_walk_box).  fpw (faces set up per wave, a power of two 4 .. 64) is the host's
//                  choice; the image depends neither on it nor on MESH_LANE_PX (integer min of a key that is a function of
//                  (face, pixel) alone).  Coverage is decided by int64 edge functions of the snapped coordinates - exact -
//                  with the top-left fill rule; depth is perspective-correct in fp64 from those integers.
// k_mesh_resolve   one thread per pixel: the core's resolve, the winning face, and with `coord` that face's edge functions
//                  again -> the interpolated unposed, unscaled vertex.
//
// The fp64 arithmetic stands in small functions with contraction off and plain operators: the __dmul_rn / __dadd_rn intrinsics
// are `*` and `+` of a header compiled with contraction on, and were fused where they met (see bop_dist, catre_bop.h).
#pragma once
#include "catre_device.h"

#include "catre_track.h"
#include "catre_zbuf.h"

constexpr int MESH_THREADS = 256;
constexpr int MESH_SNAP = 256;               // sub-pixel positions per pixel
constexpr int MESH_LANE_PX = 16;             // boxes of at most this many samples: a lane per face (k_mesh_raster)
constexpr float MESH_COORD_LIMIT = 8388608.f;  // 2^23: |xi|, |yi| below it -> differences below 2^24, products below 2^49

// the ragged mesh table (device), the instance -> mesh map and the instance-major offsets of the posed vertices and faces
struct MeshTables {
  const float* verts;            // [V_tot,3]
  const int32_t* faces;          // [T_tot,3] indices local to the mesh
  const int32_t* vert_off;       // [G+1]
  const int32_t* face_off;       // [G+1]
  const int32_t* mesh_of;        // [I]
  const int32_t* inst_vert_off;  // [I+1]
  const int32_t* inst_face_off;  // [I+1]
  int G, V_tot, T_tot, I, NV, NF;
};

// the last i in [0, n) with off[i] <= g (off ascending, off[0] == 0 <= g): the trip count depends on n alone
__device__ __forceinline__ int mesh_owner(const int32_t* __restrict__ off, int n, int g) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_mesh_project(MeshTables T, const float* __restrict__ pose, const float* __restrict__ scale,
                                                      const int* __restrict__ frame_of, const PclCam* __restrict__ cams,
                                                      int4* __restrict__ rec, int4* __restrict__ rec_out) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi >= T.NV) return;
  const int i = mesh_owner(T.inst_vert_off, T.I, gi);
  const int local = gi - T.inst_vert_off[i], m = T.mesh_of[i];
  int4 r = make_int4(0, 0, 0, 0);
  if ((unsigned)m < (unsigned)T.G && local >= 0) {
    const int vb = T.vert_off[m], vn = T.vert_off[m + 1] - vb;
    const long long row = (long long)vb + local;
    if (vb >= 0 && local < vn && row < T.V_tot) {
      const PclCam cam = cams[frame_of[i]];
      float x, y, z;
      nn_load_point(T.verts, (size_t)row, pose + (size_t)i * 12, scale + (size_t)i * 3, x, y, z);
      float u, v;
      zbuf_project(cam, x, y, z, u, v);
      const float xs = rintf(__fmul_rn(u, (float)MESH_SNAP)), ys = rintf(__fmul_rn(v, (float)MESH_SNAP));
      // decided in float: a vertex a hair in front of the camera has u beyond any int (a NaN fails every comparison)
      const bool ok = z > 0.f && track_finite(u) && track_finite(v) && fabsf(xs) < MESH_COORD_LIMIT && fabsf(ys) < MESH_COORD_LIMIT;
      r = make_int4(ok ? (int)xs : 0, ok ? (int)ys : 0, __float_as_int(z), ok ? 1 : 0);
    }
  }
  rec[gi] = r;
  if (rec_out) rec_out[gi] = r;
}

// a posed face from the records: snapped corners (oriented: area2 > 0), depths, the rows of its corners in `verts`
struct MeshFace {
  int x0, y0, x1, y1, x2, y2;
  float z0, z1, z2;
  int r0, r1, r2;
  long long area2;
};
constexpr int MESH_DRAW = 0, MESH_CULLED = 1, MESH_EMPTY = 2;

// face `local` of instance i.  Nothing is indexed before it is known to lie inside its table.
__device__ __forceinline__ int mesh_face_setup(const MeshTables& T, const int4* __restrict__ rec, int i, int local, MeshFace& f) {
  const int m = T.mesh_of[i];
  if ((unsigned)m >= (unsigned)T.G || local < 0) return MESH_CULLED;
  const int fb = T.face_off[m], fn = T.face_off[m + 1] - fb, vb = T.vert_off[m], vn = T.vert_off[m + 1] - vb;
  const long long row = (long long)fb + local;
  if (fb < 0 || local >= fn || row >= T.T_tot || vb < 0 || vn <= 0 || (long long)vb + vn > T.V_tot) return MESH_CULLED;
  const int32_t* idx = T.faces + row * 3;
  const int a = idx[0], b = idx[1], c = idx[2];
  if ((unsigned)a >= (unsigned)vn || (unsigned)b >= (unsigned)vn || (unsigned)c >= (unsigned)vn) return MESH_CULLED;
  const long long base = T.inst_vert_off[i];
  if (base < 0 || base + vn > T.NV) return MESH_CULLED;
  const int4 p0 = rec[base + a], p1 = rec[base + b], p2 = rec[base + c];
  if (!(p0.w && p1.w && p2.w)) return MESH_CULLED;
  const long long area2 = (long long)(p1.x - p0.x) * (p2.y - p0.y) - (long long)(p1.y - p0.y) * (p2.x - p0.x);
  if (area2 == 0) return MESH_EMPTY;
  const bool flip = area2 < 0;  // either winding: corners 1 and 2 change places
  f.x0 = p0.x, f.y0 = p0.y, f.z0 = __int_as_float(p0.z), f.r0 = vb + a;
  f.x1 = flip ? p2.x : p1.x, f.y1 = flip ? p2.y : p1.y, f.z1 = __int_as_float(flip ? p2.z : p1.z), f.r1 = vb + (flip ? c : b);
  f.x2 = flip ? p1.x : p2.x, f.y2 = flip ? p1.y : p2.y, f.z2 = __int_as_float(flip ? p1.z : p2.z), f.r2 = vb + (flip ? b : c);
  f.area2 = flip ? -area2 : area2;
  return MESH_DRAW;
}

// the edge a -> b of a face with area2 > 0 has its interior where E > 0: dE/dv = dx, dE/du = -dy.  top: horizontal with the
// interior at larger v; left: not horizontal with the interior at larger u.
__device__ __forceinline__ bool mesh_top_left(int dx, int dy) { return dy < 0 || (dy == 0 && dx > 0); }
__device__ __forceinline__ long long mesh_edge(int ax, int ay, int bx, int by, int sx, int sy) {
  return (long long)(bx - ax) * (sy - ay) - (long long)(by - ay) * (sx - ax);
}
// edge functions of the sample (sx, sy), e_k opposite corner k (e0 + e1 + e2 == area2); true: the sample is the face's
__device__ __forceinline__ bool mesh_cover(int x0, int y0, int x1, int y1, int x2, int y2, int sx, int sy, long long& e0,
                                           long long& e1, long long& e2) {
  e0 = mesh_edge(x1, y1, x2, y2, sx, sy);
  e1 = mesh_edge(x2, y2, x0, y0, sx, sy);
  e2 = mesh_edge(x0, y0, x1, y1, sx, sy);
  return (e0 > 0 || (e0 == 0 && mesh_top_left(x2 - x1, y2 - y1))) && (e1 > 0 || (e1 == 0 && mesh_top_left(x0 - x2, y0 - y2))) &&
         (e2 > 0 || (e2 == 0 && mesh_top_left(x1 - x0, y1 - y0)));
}

__device__ __forceinline__ double mesh_rcp(float z) {
#pragma clang fp contract(off)
  return 1.0 / (double)z;
}
// w_k = E_k * (1 / z_k), W = (w_0 + w_1) + w_2
__device__ __forceinline__ double mesh_weights(long long e0, long long e1, long long e2, double rz0, double rz1, double rz2,
                                               double& w0, double& w1, double& w2) {
#pragma clang fp contract(off)
  w0 = (double)e0 * rz0;
  w1 = (double)e1 * rz1;
  w2 = (double)e2 * rz2;
  const double s = w0 + w1;
  return s + w2;
}
__device__ __forceinline__ float mesh_depth(long long area2, double W) {
#pragma clang fp contract(off)
  const double z = (double)area2 / W;
  return (float)z;
}
// ((w_0 a_0 + w_1 a_1) + w_2 a_2) / W
__device__ __forceinline__ float mesh_attr(double w0, double w1, double w2, double W, float a0, float a1, float a2) {
#pragma clang fp contract(off)
  const double p0 = w0 * (double)a0, p1 = w1 * (double)a1, p2 = w2 * (double)a2;
  const double s = p0 + p1;
  const double t = s + p2;
  const double q = t / W;
  return (float)q;
}

// one sample of one face: covered -> depth -> key -> zbuf_min
__device__ __forceinline__ void mesh_shade(int x0, int y0, int x1, int y1, int x2, int y2, double rz0, double rz1, double rz2,
                                           long long area2, unsigned g, unsigned long long* kf, int W, int c256, int px, int py) {
  long long e0, e1, e2;
  if (mesh_cover(x0, y0, x1, y1, x2, y2, px * MESH_SNAP + c256, py * MESH_SNAP + c256, e0, e1, e2)) {
    double w0, w1, w2;
    const double Wn = mesh_weights(e0, e1, e2, rz0, rz1, rz2, w0, w1, w2);
    zbuf_min(kf + (size_t)py * W + px, zbuf_key(mesh_depth(area2, Wn), g));
  }
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_raster(MeshTables T, const int4* __restrict__ rec,
                                                              const int* __restrict__ frame_of, int fpw, int c256, int H, int W,
                                                              unsigned long long* keys, int32_t* culled) {
  const int tid = threadIdx.x, lane = tid & 63;
  const long long gl = ((long long)blockIdx.x * (MESH_THREADS / 64) + (tid >> 6)) * fpw + lane;
  // this lane's face: bounding box [bx, bx + bw) x [by, by + bh) in pixels, bw == 0 = nothing to draw
  int bx = 0, by = 0, bw = 0, bh = 0, frame = 0;
  MeshFace f = {};
  double rz0 = 0., rz1 = 0., rz2 = 0.;
  if (lane < fpw && gl < T.NF) {
    const int g = (int)gl, i = mesh_owner(T.inst_face_off, T.I, g);
    const int st = mesh_face_setup(T, rec, i, g - T.inst_face_off[i], f);
    if (st == MESH_CULLED) atomicAdd(culled + i, 1);
    if (st == MESH_DRAW) {
      // samples 256 p + c256 inside the corners' extent, clamped to the image: no trip count depends on unclamped data
      const int xmin = min(f.x0, min(f.x1, f.x2)), xmax = max(f.x0, max(f.x1, f.x2));
      const int ymin = min(f.y0, min(f.y1, f.y2)), ymax = max(f.y0, max(f.y1, f.y2));
      const int ulo = max((xmin - c256 + MESH_SNAP - 1) >> 8, 0), uhi = min((xmax - c256) >> 8, W - 1);
      const int vlo = max((ymin - c256 + MESH_SNAP - 1) >> 8, 0), vhi = min((ymax - c256) >> 8, H - 1);
      if (ulo <= uhi && vlo <= vhi) {
        bx = ulo;
        by = vlo;
        bw = uhi - ulo + 1;
        bh = vhi - vlo + 1;
        frame = frame_of[i];
        rz0 = mesh_rcp(f.z0);
        rz1 = mesh_rcp(f.z1);
        rz2 = mesh_rcp(f.z2);
      }
    }
  }
  // a face whose box holds at most MESH_LANE_PX samples is drawn by its own lane, all such faces of the wave side by side
  if (bw > 0 && bw * bh <= MESH_LANE_PX) {
    unsigned long long* kf = keys + (size_t)frame * H * W;
    const int total = bw * bh;
    int u = 0, v = 0;
    for (int k = 0; k < total; ++k) {
      mesh_shade(f.x0, f.y0, f.x1, f.y1, f.x2, f.y2, rz0, rz1, rz2, f.area2, (unsigned)gl, kf, W, c256, bx + u, by + v);
      if (++u == bw) {
        u = 0;
        ++v;
      }
    }
    bw = 0;
  }
  zbuf_each_live(bw > 0, [&](int j) {
    const int jbx = zbuf_bcast(bx, j), jby = zbuf_bcast(by, j), jbw = zbuf_bcast(bw, j), jbh = zbuf_bcast(bh, j);
    const int x0 = zbuf_bcast(f.x0, j), y0 = zbuf_bcast(f.y0, j), x1 = zbuf_bcast(f.x1, j), y1 = zbuf_bcast(f.y1, j);
    const int x2 = zbuf_bcast(f.x2, j), y2 = zbuf_bcast(f.y2, j);
    const double jr0 = zbuf_bcast(rz0, j), jr1 = zbuf_bcast(rz1, j), jr2 = zbuf_bcast(rz2, j);
    const long long area2 = zbuf_bcast(f.area2, j);
    const unsigned jg = (unsigned)zbuf_bcast((int)gl, j);
    unsigned long long* kf = keys + (size_t)zbuf_bcast(frame, j) * H * W;
    zbuf_walk_box(lane, jbx, jby, jbw, jbh, [&](int px, int py) {
      mesh_shade(x0, y0, x1, y1, x2, y2, jr0, jr1, jr2, area2, jg, kf, W, c256, px, py);
    });
  });
}

__global__ __launch_bounds__(256) void k_mesh_resolve(MeshTables T, const int4* __restrict__ rec,
                                                      const unsigned long long* __restrict__ keys,
                                                      const float* __restrict__ depth, float delta, int n, int c256, int H, int W,
                                                      int32_t* __restrict__ labels, float* __restrict__ zbuf,
                                                      int32_t* __restrict__ face, unsigned char* __restrict__ cls,
                                                      int32_t* __restrict__ labels_fit, int32_t* __restrict__ counts,
                                                      float* __restrict__ coord) {
  const int gi = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  int code = -1;
  if (gi < n) {
    const unsigned long long key = keys[gi];
    const bool bg = key == ZBUF_BG;
    const int g = (int)zbuf_key_lo(key);
    const int inst = bg ? 0 : mesh_owner(T.inst_face_off, T.I, g);
    const int local = bg ? -1 : g - T.inst_face_off[inst];
    code = zbuf_resolve_pixel(key, inst, depth, delta, gi, labels, zbuf, cls, labels_fit, [&] {
      if (face) face[gi] = local;
    });
    if (coord) {
      float cx = 0.f, cy = 0.f, cz = 0.f;
      MeshFace f;
      if (!bg && mesh_face_setup(T, rec, inst, local, f) == MESH_DRAW) {
        const int px = gi % W, py = (gi / W) % H;
        long long e0, e1, e2;
        mesh_cover(f.x0, f.y0, f.x1, f.y1, f.x2, f.y2, px * MESH_SNAP + c256, py * MESH_SNAP + c256, e0, e1, e2);
        double w0, w1, w2;
        const double Wn = mesh_weights(e0, e1, e2, mesh_rcp(f.z0), mesh_rcp(f.z1), mesh_rcp(f.z2), w0, w1, w2);
        const float *a0 = T.verts + (size_t)f.r0 * 3, *a1 = T.verts + (size_t)f.r1 * 3, *a2 = T.verts + (size_t)f.r2 * 3;
        cx = mesh_attr(w0, w1, w2, Wn, a0[0], a1[0], a2[0]);
        cy = mesh_attr(w0, w1, w2, Wn, a0[1], a1[1], a2[1]);
        cz = mesh_attr(w0, w1, w2, Wn, a0[2], a1[2], a2[2]);
      }
      coord[(size_t)gi * 3] = cx;
      coord[(size_t)gi * 3 + 1] = cy;
      coord[(size_t)gi * 3 + 2] = cz;
    }
  }
  zbuf_count(code, lane, counts);
}
