// Host side of the z-buffer core (catre_zbuf.h): what the C ABI of the splat render and of the mesh rasteriser share
namespace {
// pixels are indexed by one int across all frames
inline bool splat_frames_ok(int F, int H, int W) {
  return F > 0 && H > 0 && W > 0 && (size_t)F * (size_t)H * (size_t)W < ((size_t)1 << 30);
}
// the staged tables: [F] cameras (4 floats each), then frame_of for at most `cap` instances
inline size_t zbuf_tab_ints(int F, size_t cap) { return (size_t)F * 4 + cap; }
struct ZbufTables {
  const PclCam* cams;
  const int* frame_of;
};
// one host->device copy of the tables to `tab` (pageable source: the runtime has consumed it when the call returns)
inline int zbuf_stage(int* tab, const float* K, const int32_t* frame_of, int F, int I, hipStream_t st, ZbufTables& T) {
  std::vector<int> head(zbuf_tab_ints(F, I));
  for (int f = 0; f < F; ++f) {
    const PclCam cam = pcl_cam(K + f * 9);
    memcpy(&head[(size_t)f * 4], &cam, sizeof cam);
  }
  for (int i = 0; i < I; ++i) head[(size_t)F * 4 + i] = frame_of[i];
  if (hipMemcpyAsync(tab, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) return CATRE_ERR_LAUNCH;
  T = ZbufTables{(const PclCam*)tab, tab + (size_t)F * 4};
  return CATRE_OK;
}
// items (points, faces) a wave takes on: 64 where that still gives every SIMD of the chip several waves (4096 in all), fewer -
// down to 4 - for a handful of items, which then spread over more waves.  A power of two; the image does not depend on it.
inline int zbuf_items_per_wave(size_t items) {
  const size_t per = items / 4096;
  int ipw = 4;
  while (ipw < 64 && (size_t)ipw * 2 <= per) ipw *= 2;
  return ipw;
}
}  // namespace
