#!/bin/bash
# the GPU kernel / segmentation / embedding tests under the CHECKED library (csrc/checked.h): every DZN_CHECK in the hand-scheduled
# kernels is live; tests/conftest.py fails the session if one fired.  Build first: python -m diarizen_amd.build --checked
export DZN_HIP_LIB="$(pwd)/diarizen_amd/lib/libdzn_hip_checked.so"
mkdir -p gpurun_out
rm -f gpurun_out/checked_build_status.txt
python -m pytest tests/test_ops_gpu.py tests/test_seg_gpu.py tests/test_emb_gpu.py -m gpu -q -x -k "not linkage and not vbx and not cdist and not clustering" 2>&1 | tail -15 > gpurun_out/${DZN_CHECKED_LOG:-r6_checked_build.log}
# the per-speaker score kernels (post.hip, ids 0x81x): a session of its own, its status line joins the first one's below
python -m pytest tests/test_scores_gpu.py -m gpu -q -x 2>&1 | tail -3
# the device resampler (resample.hip, ids 0x82x): likewise
python -m pytest tests/test_resample_gpu.py tests/test_telephony_gpu.py -m gpu -q -x 2>&1 | tail -3
# detection: whole-recording and range form, and the stream on top of it (post.hip, ids 0x80x): likewise
python -m pytest tests/test_detection_gpu.py tests/test_detection_stream_op_gpu.py tests/test_detection_stream_gpu.py tests/test_diarize_range_gpu.py -m gpu -q -x 2>&1 | tail -3
# the contraction tile matrix (gemm*.hip, ids 0x10x / 0x20x / 0x30x: scale-unit indices against amax_count, ring stages): likewise
python -m pytest tests/test_gemm_tiles_gpu.py -m gpu -q -x 2>&1 | tail -3
# the attention matrix (attention_split.hip, attention_planes.hip, ids 0x60x / 0x61x: staged tiles inside their planes): likewise
python -m pytest tests/test_attention_matrix_gpu.py -m gpu -q -x 2>&1 | tail -3
# the small-kernel matrix (conformer.hip, frontend.hip, norm.hip, embed.hip through their dzn_op_* entry points): likewise
python -m pytest tests/test_small_kernels_gpu.py -m gpu -q -x 2>&1 | tail -3
# the image-kernel matrix (conv_split.hip, resblock_fused.hip, resblock_ws.hip, ids 0x40x / 0x50x: image indices of the lists, ring rows): likewise
python -m pytest tests/test_image_kernels_gpu.py -m gpu -q -x 2>&1 | tail -3
# the front-end matrix (frontend.hip, frontend_fused.hip, ids 0x71x: plane rows, conv1 fragments, weight fragments): likewise
python -m pytest tests/test_frontend_kernels_gpu.py -m gpu -q -x 2>&1 | tail -3
# engine reuse (one oversize handle, many shapes: tracker indices m / L against max_batch entries, tile offsets, the last key tile
# of the plane attention): likewise
python -m pytest tests/test_engine_reuse_gpu.py -m gpu -q -x 2>&1 | tail -3
# the beamformer (beamform.hip, ids 0x85x: frame and shifted sample reads against the span given, butterfly / twiddle indices): likewise
python -m pytest tests/test_beamform_gpu.py -m gpu -q -x 2>&1 | tail -3
# live array feeds (beamform_live.hip, ids 0x86x: planar frame rows, tracker columns; beamform.hip's reads against the uploaded span): likewise
python -m pytest tests/test_beamform_live_gpu.py -m gpu -q -x 2>&1 | tail -3
# array feeds in the hub (beamform_many.hip, ids 0x87x: tiles and work items of their descriptors, the carried samples; the
# 0x85x / 0x86x checks of beamform_tile.h against the wave's scratch and the rows' tables): likewise
python -m pytest tests/test_beamform_many_gpu.py tests/test_hub_array_gpu.py -m gpu -q -x 2>&1 | tail -3
# live per-speaker scores (post.hip, ids 0x833 / 0x834: the soft row read and the score write of the fused range kernel): likewise
python -m pytest tests/test_live_scores_gpu.py -m gpu -q -x 2>&1 | tail -3
# the resegmentation matching (reseg.hip, ids 0x88x: decision / reference reads, LDS words, the count write); its word is read by
# the test itself (dzn_checked_collect_reseg), not by dzn_checked_status
python -m pytest tests/test_resegmentation_gpu.py -m gpu -q -x 2>&1 | tail -3
# the speaker registry (registry.hip, ids 0x8ax: member index, row reads, LDS tile, segment and table writes); its word is read
# by the test itself (dzn_checked_collect_registry)
python -m pytest tests/test_registry_gpu.py -m gpu -q -x 2>&1 | tail -3
cat gpurun_out/checked_build_status.txt >> gpurun_out/${DZN_CHECKED_LOG:-r6_checked_build.log}
tail -6 gpurun_out/${DZN_CHECKED_LOG:-r6_checked_build.log}
