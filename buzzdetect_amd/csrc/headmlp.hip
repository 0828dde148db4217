// The dense-stack classifier head (include/buzzdetect_head.h).  A lone stack is a set of heads of one member: bd_head_attach
// builds it with headset.hip's builder (fused route off) and the pass runs it with the set's kernels - one launch per Dense layer,
// C[W][N] = act(A[W][K] W + b), in exact float32 on v_mfma_f32_32x32x2_f32, whatever arithmetic the CNN runs in; a softmax is a
// row pass behind the last layer.  What lives here is the bd_head_* exports and the packed operand format, which headset.hip,
// simsearch.hip and cluster.hip share (dense_pack_weights; the walk that reads it is dense_tile_walk in dense_device.h).
//
// A wave owns one 32 x 32 tile of C and walks K alone, in ascending super-steps of 8 k: nothing is split over waves or
// workgroups and nothing is added atomically, and the instruction is a chain of fused multiply-adds per output element, so an
// output depends on its row of A, its column of W and the walk's k order only - not on where the row sits in the launch.
// That is what lets a window give the same bits alone, inside a full pass and inside a ragged last pass.
//
// Operand map (cnn.hip, pointwise_kernel): lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; lane-half h
// takes k = 8 s + 4 h + j for the j-th instruction of super-step s, so one 16-byte load per operand feeds four instructions.
//   A  straight from global memory: row min(row, W - 1) (always in bounds, never stored), 16 bytes at k = 8 s + 4 h.  Rows are
//      lda >= round_up(K, 32) floats apart, so the load stays inside its row; elements at k >= K (never written: the layer
//      before stores its N columns only) are replaced by zero.
//   B  the host packs W into fragment order at attach time, zero-padded to 32-column tiles and 32-k groups:
//      [N / 32 tiles][K / 8 super-steps][64 lanes][4]: lane l holds W[8 s + 4 (l >> 5) + j][32 t + (l & 31)], j = 0..3.
//      A wave's load of a super-step is 1 KB, contiguous.
// Four super-steps (32 k) are in flight ahead of the sixteen matrix instructions that use them; one accumulator per wave is
// enough, the instruction's issue interval and its dependent latency both being 64 cycles.  A workgroup is 2 x 2 waves = a
// 64 x 64 tile, so 1024 windows x 1024 columns are 256 workgroups, one per compute unit.  There is no LDS and no barrier.
#include "engine_state.h"

#include "../../include/buzzdetect_head.h"
#include "../../include/buzzdetect_headset.h"

namespace bd {

size_t dense_packed_floats(int k, int n) { return (size_t)((k + 31) / 32 * 32) * ((n + 31) / 32 * 32); }

void dense_pack_weights(const float* kernel, int k, int n, float* dst) {
    const int n_super = (k + 31) / 32 * 4, tiles = (n + 31) / 32;
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < n_super; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                    const int kk = 8 * s + 4 * (l >> 5) + j, nn = 32 * t + (l & 31);
                    dst[(((size_t)t * n_super + s) * 64 + l) * 4 + j] = kk < k && nn < n ? kernel[(size_t)kk * n + nn] : 0.0f;
                }
}

}  // namespace bd

extern "C" {

int bd_head_abi_version(void) { return BD_HEAD_ABI_VERSION; }

int bd_head_outputs(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_head_outputs: null handle");
    return h->set.lone ? h->set.outputs : 0;
}

int bd_head_attach(bd_handle h, const bd_head_layer* layers, int32_t n_layers) {
    if (!h || !layers) return fail(BD_EINVAL, "bd_head_attach: null argument");
    if (h->n_classes != 0)
        return fail(BD_EINVAL, "bd_head_attach: the engine already has a head (create it with n_classes == 0)");
    BD_HIP(hipSetDevice(h->device));
    const bd_headset_member member = {layers, n_layers, 0};
    std::string err;
    bd::HeadSet set;
    const int rc = bd::headset_build(&member, 1, true, &set, &err);
    if (rc != BD_OK) return fail(rc, err);
    h->set = std::move(set);
    h->n_classes = h->set.outputs;
    return BD_OK;
}

}  // extern "C"
