// gemm_launch.h — what the contraction families (gemm.hip, gemm_split.hip, gemm_split_pre.hip, gemm_mx.hip) share around
// their main loops: the tile override, the host launcher and the device prologue.  A change to the launch path or to the
// tile / batch decode is made here, once.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "common.h"

// A tile shape forced by name: read from its environment variable on first use, rewritten by its setter (tuning scripts
// and tests walk several shapes in one process); "auto", "" or NULL clear it.  What a name means is up to the family that
// reads it; a name a family does not know leaves its shape rule in charge.
class TileOverride {
 public:
  explicit TileOverride(const char* env) : env_(env) {}
  const char* get() {
    if (!init_) set(getenv(env_));
    return buf_[0] ? buf_ : nullptr;
  }
  void set(const char* cfg) {
    init_ = true;
    snprintf(buf_, sizeof(buf_), "%s", cfg && strcmp(cfg, "auto") ? cfg : "");
  }

 private:
  const char* env_;
  char buf_[32] = {0};
  bool init_ = false;
};
inline TileOverride g_gemm_cfg{"DZN_GEMM_CFG"};         // plain, split and pre-split families (dzn_op_set_gemm_cfg)
inline TileOverride g_gemm_mx_cfg{"DZN_GEMM_MX_CFG"};   // gemm_mx.hip: its names denote other kernels (dzn_op_set_gemm_mx_cfg)

// DZN_NO_H2: the fp16 two-term / MX forms stand down for the bf16 three-term kernel
inline bool gemm_no_h2() {
  static const bool v = getenv("DZN_NO_H2") != nullptr;
  return v;
}

// Partials per row (column tiles x wavefront columns) that the last contraction launched by this thread with stat_partial set
// left: what a caller that reduces the partials itself (stat_final == NULL) passes on as their count.  Known only here,
// where the tile has been chosen.
inline thread_local int g_stat_partials_last = 0;

// profiler record of one contraction launch: class gemm_<tag>_<BM>x<BN>, by shape under DZN_PROFILE_SHAPES
inline int gemm_prof_begin(const dzn_gemm_desc& d, hipStream_t s, const char* tag, int BM, int BN, int w_bytes_per_elem) {
  if (!prof_enabled()) return -1;
  static const bool by_shape = getenv("DZN_PROFILE_SHAPES") != nullptr;
  char cls[64];
  if (by_shape) snprintf(cls, sizeof(cls), "gemm_%s_%dx%d M%d N%d K%d z%d", tag, BM, BN, d.M, d.N, d.K, d.nz);
  else snprintf(cls, sizeof(cls), "gemm_%s_%dx%d", tag, BM, BN);
  const double fl = d.alg_flops > 0 ? d.alg_flops * d.nz : 2.0 * d.M * d.N * d.K * d.nz;
  return prof_begin(s, cls, fl, gemm_alg_bytes(d, w_bytes_per_elem));
}

// One launch of contraction kernel KERN (BM x BN tiles, WGN wavefront columns per tile, `threads` per workgroup, `lds` bytes
// of dynamic LDS): one workgroup per tile x nz grid rows, the profiler record, and the reduction of the epilogue's row
// statistics where the descriptor asks for them.  `extra` = kernel arguments behind the descriptor.
template <auto KERN, typename... Extra>
int launch_contraction(const dzn_gemm_desc& d, hipStream_t s, int threads, size_t lds, int BM, int BN, int WGN, const char* tag,
                       int w_bytes_per_elem, Extra... extra) {
  const int tilesM = (d.M + BM - 1) / BM, tilesN = (d.N + BN - 1) / BN;
  static unsigned long long attr_mask = 0;  // one bit per HIP device (function attributes are per device), one mask per kernel
  if (first_use_on_device(attr_mask))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const int pid = gemm_prof_begin(d, s, tag, BM, BN, w_bytes_per_elem);
  hipLaunchKernelGGL(KERN, dim3(tilesM * tilesN, d.nz > 0 ? d.nz : 1, 1), dim3(threads), lds, s, d, extra...);
  prof_end(pid, s);
  if (hipGetLastError() != hipSuccess) return DZN_E_HIP;
  if (d.stat_partial) g_stat_partials_last = tilesN * WGN;
  if (d.stat_partial && d.stat_final)
    return launch_stats_finalize(d.stat_partial, d.M, tilesN * WGN, d.stat_C, d.stat_eps, d.stat_final, s);
  return DZN_OK;
}

// Device prologue: workgroup -> (row tile tm, column tile tn) and grid row -> (z0, z1).  Workgroup ids are remapped so that
// each XCD (private L2) walks a contiguous run of tiles (bijective for any grid size).  false = this workgroup has no work:
// its z0 lies outside the device-chosen subset of the batch (dzn_gemm_desc.z_count / z_list).
__device__ __forceinline__ bool gemm_tile(const dzn_gemm_desc& d, const int tilesN, int& tm, int& tn, int& z0, int& z1) {
  int t;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  tm = t / tilesN;
  tn = t % tilesN;
  const int z = blockIdx.y;
  z0 = z / d.zdiv;
  z1 = z - z0 * d.zdiv;
  if (d.z_list) {
    if (z0 >= d.z_count[0]) return false;
    z0 = d.z_list[z0];
  }
  return true;
}
