// C ABI of the mesh rasteriser (kernels: catre_mesh.h; shared host side: catre_zbuf_api.inc; declarations: include/catre_hip.h)
namespace {
constexpr int MESH_MAX_I = 1 << 27;  // instance * 8 + class is one int in the resolve
// [F*H*W] 64-bit keys, [NV] vertex records of 16 bytes, then the staged tables with frame_of sized for the most instances NV
// vertices can belong to (every mesh has a vertex), so that the workspace depends on the frames and the posed vertices alone
struct MeshWs {
  size_t keys_bytes, rec_bytes, total_bytes;
};
inline MeshWs mesh_ws(int F, int H, int W, int NV) {
  MeshWs L;
  L.keys_bytes = align_up((size_t)F * H * W * 8, 16);  // the records are read and written 16 bytes at a time
  L.rec_bytes = (size_t)NV * 16;
  L.total_bytes = align_up(L.keys_bytes + L.rec_bytes + zbuf_tab_ints(F, (size_t)NV) * sizeof(int), 256);
  return L;
}
}  // namespace

size_t catre_mesh_workspace_bytes(int F, int H, int W, int n_posed_vertices) {
  return splat_frames_ok(F, H, W) && n_posed_vertices > 0 ? mesh_ws(F, H, W, n_posed_vertices).total_bytes : 0;
}

int catre_mesh_render(const float* verts, const int32_t* faces, const int32_t* vert_off, const int32_t* face_off,
                      const int32_t* mesh_of, const int32_t* inst_vert_off, const int32_t* inst_face_off, const float* pose,
                      const float* scale, const float* depth, const float* K, const int32_t* frame_of, float delta,
                      int pixel_center_half, int G, int V_tot, int T_tot, int F, int I, int n_posed_vertices, int n_posed_faces,
                      int H, int W, void* workspace, size_t ws_bytes, int32_t* labels, float* zbuf, int32_t* face,
                      unsigned char* cls, int32_t* labels_fit, int32_t* counts, int32_t* culled, float* coord,
                      int32_t* projected, void* stream) {
  REQUIRE(verts && faces && vert_off && face_off && mesh_of && inst_vert_off && inst_face_off && pose && scale && K && frame_of);
  REQUIRE(labels && zbuf && counts && culled);
  REQUIRE(G > 0 && V_tot > 0 && T_tot > 0 && I > 0 && n_posed_vertices >= I && n_posed_faces >= I && splat_frames_ok(F, H, W));
  REQUIRE(delta == delta && (pixel_center_half == 0 || pixel_center_half == 1));
  if (I > MESH_MAX_I) return CATRE_ERR_UNSUPPORTED;
  REQUIRE(pclf_tables_ok(K, frame_of, F, I));
  const int NV = n_posed_vertices, NF = n_posed_faces;
  const MeshWs L = mesh_ws(F, H, W, NV);
  if (!workspace || ws_bytes < L.total_bytes) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  int4* rec = (int4*)((char*)workspace + L.keys_bytes);
  ZbufTables tab;
  if (const int err = zbuf_stage((int*)((char*)workspace + L.keys_bytes + L.rec_bytes), K, frame_of, F, I, st, tab)) return err;
  const MeshTables T{verts, faces, vert_off, face_off, mesh_of, inst_vert_off, inst_face_off, G, V_tot, T_tot, I, NV, NF};
  const int n = F * H * W, c256 = pixel_center_half ? MESH_SNAP / 2 : 0;
  const int fpw = zbuf_items_per_wave((size_t)NF), per_block = (MESH_THREADS / 64) * fpw;
  hipLaunchKernelGGL(k_zbuf_clear, dim3((std::max(n, I * 5) + 255) / 256), dim3(256), 0, st, keys, n, counts, I * 5, culled, I);
  hipLaunchKernelGGL(k_mesh_project, dim3((NV + 255) / 256), dim3(256), 0, st, T, pose, scale, tab.frame_of, tab.cams, rec,
                     (int4*)projected);
  hipLaunchKernelGGL(k_mesh_raster, dim3((unsigned)(((long long)NF + per_block - 1) / per_block)), dim3(MESH_THREADS), 0, st, T,
                     (const int4*)rec, tab.frame_of, fpw, c256, H, W, keys, culled);
  hipLaunchKernelGGL(k_mesh_resolve, dim3((n + 255) / 256), dim3(256), 0, st, T, (const int4*)rec,
                     (const unsigned long long*)keys, depth, delta, n, c256, H, W, labels, zbuf, face, cls, labels_fit, counts,
                     coord);
  return check_launch();
}
