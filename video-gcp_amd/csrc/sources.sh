# Sources of libgcpx.so and their per-file flags — the ONE list csrc/build.sh, tools/build_variant.sh and tools/isa_hazard_scan.py read.
GCPX_SOURCES="conv3x3 conv3x3_split conv3x3_lowres conv3x3_head_split conv3x3_head32 conv_enc conv_enc_split conv_enc_fused gemm gemm_split gemm_planes mlp mlp_bwd misc loss wgrad wgrad_conv wgrad_conv_split wgrad_rows_split wgrad_image split_pack backward scalar_f32 adaptive aux metrics comm batch_assemble topdown_traj topn panel train_stats prm nav_env tree_search cem_batch enc_frames"
# built without SLP vectorisation = without packed-f32 VALU instructions (profiles/r05_head_store_hazard.txt, scalar_f32.hip)
GCPX_NO_SLP="conv3x3_head_split conv3x3_head32 loss scalar_f32"
# built without contraction of a multiply and an add into an FMA: results defined as separately rounded float32 operations (cem_batch.hip)
GCPX_NO_CONTRACT="cem_batch"
GCPX_HEADERS="common.h resize_passes.h gemm_tile.h split_tr.h split_mfma.h split_common.h ../../include/gcpx.h"
gcpx_flags_for() {
  for s in $GCPX_NO_SLP; do if [ "$s" = "$1" ]; then echo "-fno-slp-vectorize"; return; fi; done
  for s in $GCPX_NO_CONTRACT; do if [ "$s" = "$1" ]; then echo "-ffp-contract=off"; return; fi; done
  echo ""
}
