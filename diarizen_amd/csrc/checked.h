// checked.h — the CHECKED build (python -m diarizen_amd.build --checked  ->  lib/libdzn_hip_checked.so, -DDZN_CHECKED).
//
// ~60 hand-scheduled kernels with raw s_waitcnt / s_barrier pipelines, LDS-DMA fills and XOR-swizzled LDS images: an index that
// leaves its LDS stage, a tracker read past its array (r4 found one by accident: a B = 1 conv launch indexed its |max| tracker by
// m / L) or a tile that walks off the descriptor does not fault on this hardware — it reads whatever lies there.  In a checked
// build the kernels carry DZN_CHECK(cond, id, detail) at those index computations.  A failed check does NOT trap (a trap kills
// the context and every later test with it): it counts itself in a per-translation-unit device word — the first failure also
// records its id, workgroup and a detail value — and the run goes on.  dzn_checked_status() (engine.cpp) sums the words of all
// translation units; tests/conftest.py fails the session when it is non-zero (scripts/run_checked.sh ->
// profiles/r5_checked_build.log).  Release builds compile the macro to nothing.
//
// Device symbols are per translation unit (the library is not built with relocatable device code): every .hip file that uses
// DZN_CHECK instantiates its word with DZN_CHECKED_TU(name), which also defines the host-side collector that engine.cpp calls.
#pragma once
#include <hip/hip_runtime.h>

#ifdef DZN_CHECKED
#define DZN_CHECKED_TU(name)                                                                                     \
  namespace { __device__ unsigned int dzn_check_word_[4] = {0u, 0u, 0u, 0u}; }                                    \
  extern "C" int dzn_checked_collect_##name(unsigned int* out4, int reset) {                                     \
    unsigned int z[4] = {0u, 0u, 0u, 0u};                                                                         \
    if (hipDeviceSynchronize() != hipSuccess) return -3;                                                          \
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(dzn_check_word_), sizeof(z)) != hipSuccess) return -3;               \
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(dzn_check_word_), z, sizeof(z)) != hipSuccess) return -3;           \
    return 0;                                                                                                     \
  }
#define DZN_CHECK(cond, id, detail)                                                                              \
  do {                                                                                                            \
    if (!(cond)) {                                                                                                \
      if (atomicAdd(&dzn_check_word_[0], 1u) == 0u) {                                                             \
        dzn_check_word_[1] = (unsigned)(id);                                                                      \
        dzn_check_word_[2] = blockIdx.x;                                                                          \
        dzn_check_word_[3] = (unsigned)(detail);                                                                  \
      }                                                                                                           \
    }                                                                                                             \
  } while (0)
#else
#define DZN_CHECKED_TU(name)
#define DZN_CHECK(cond, id, detail) do { } while (0)
#endif

// check ids: 0x1xx gemm_split, 0x2xx gemm_mx, 0x3xx gemm_split_pre, 0x4xx resblock_fused, 0x5xx resblock_ws,
//            0x60x attention_split, 0x61x attention_planes, 0x7xx frontend_fused, 0x80x post (detection), 0x81x post (speaker scores),
//            0x82x resample / decode / ingest (0x828 ..), 0x83x post (diarize range),
//            0x84x gallery (0x840 row-tile index, 0x841 partial-list write, 0x842 survivor queue),
//            0x85x beamform (0x850 frame read, 0x852 / 0x853 butterfly and twiddle index, 0x854 block, 0x855 lag read,
//                            0x858 delay read, 0x859 shifted sample read, 0x85a output write),
//            0x86x beamform_live (0x860 planar frame read / write, 0x862 tracker column),
//            0x87x beamform_many (0x870 decode tile of its descriptor, 0x871 format, 0x872 GCC work item and LDS image,
//                                 0x873 channel of the item, 0x874 tracker descriptor, 0x875 sum tile, 0x876 carried sample);
//            the 0x85x / 0x86x checks of beamform_tile.h count in the translation unit that includes it;
//            0x88x reseg (0x880 decision read, 0x881 reference read, 0x882 LDS word, 0x883 count write) — its collector
//            dzn_checked_collect_reseg is read by tests/test_resegmentation_gpu.py, dzn_checked_status does not sum it;
//            0x89x linkage, pdist_cosine_group_kernel (0x890 LDS stage index, 0x891 embedding read, 0x892 norm / group read,
//            0x893 matrix write) — its collector dzn_checked_collect_linkage is read by tests/test_linking_gpu.py the same way;
//            0x8ax registry (0x8a0 chunk of the member index, 0x8a1 stored row number, 0x8a2 segment id, 0x8a3 row read,
//            0x8a4 LDS tile word, 0x8a5 segment-maximum write, 0x8a6 segment range of a column, 0x8a7 table write,
//            0x8a8 triple slot) — its collector dzn_checked_collect_registry is read by tests/test_registry_gpu.py the same way
