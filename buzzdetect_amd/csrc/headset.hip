// The heads attached to an engine (include/buzzdetect_headset.h, include/buzzdetect_head.h): M members, each a stack of Dense
// layers, whose outputs land side by side in the logits.  A lone stack (bd_head_attach, headmlp.hip) is a set of one member that
// never takes the fused route.  Launches per pass do not grow with M:
//
//   dense_set_kernel    one launch per DEPTH: the layer at that depth of every stack-route member.  blockIdx.y walks a tile
//                       table built at attach time: every 64-column workgroup tile of every such layer names its layer
//                       descriptor (where A is, K, the packed fragments, the bias, N, the activation, where C goes).  A wave
//                       owns one 32 x 32 tile of C and walks K alone (dense_device.h), so an output depends on its row of A, its
//                       column of W and the k order only: a member has the bits of the same stack attached alone.
//   softmax_set_kernel  one launch for every member that ends in a softmax, one wave per row (dense_device.h: softmax_row).
//   head_set_kernel     one launch for the members of the fused kind (one linear layer of at most BD_MAX_CLASSES outputs): their
//                       classes are concatenated and cut into groups of at most 64, grid (window, group); a class is computed
//                       as pool_head_kernel<1> (cnn.hip) computes it - per thread fmaf(s.x, w.x, fmaf(s.y, w.y, fmaf(s.z, w.z,
//                       s.w * w.w))) over its float4 of the embedding, an xor butterfly over the wave, ((p0 + p1) + (p2 + p3)) +
//                       bias over the four waves - and depends on no other class, so the grouping changes nothing.
//
// Scratch (bd_internal.h: kHeadSetRegions rows of kHeadSetRow floats per window, inside the workspace of the pass):
// depth d reads region (d - 1) & 1 and writes region d & 1, every layer in a 32-aligned column block of its own (A's 16-byte
// loads reach round_up(K, 32) columns; those at k >= K are replaced by zero, never used); a last layer in front of a softmax
// writes region 2, packed, where no later depth writes; every other last layer writes its member's columns of the logits.
// Nothing is split over workgroups, nothing is added atomically, every launch is idempotent.
#include "engine_state.h"
#include "dense_device.h"

#include <cstring>

#include "../../include/buzzdetect_headset.h"

namespace bd {
namespace {

enum { kFromPooled = 0, kFromScratch = 1 };
enum { kToLogits = 0, kToScratch = 1, kToSoftmax = 2 };

struct SetLayer {
    int a_src, a_col, lda;       // kFromPooled: the embeddings, lda 1024; kFromScratch: column block of the region read
    int k, n_super, n, act;
    int c_dst, c_col, ldc;
    int bias_off;                // floats from the parameter block
    long long wf_off;            // floats from the parameter block (a multiple of 4)
};
struct SetTile {
    int layer, tile;             // index into the depth's SetLayer[], 64-column tile of that layer
};
struct SetSoftmax {
    int x_col, n, y_col;         // columns of region 2, width, first column of the logits
};

__global__ __launch_bounds__(256) void dense_set_kernel(const float* __restrict__ pooled, const float* __restrict__ sin,
                                                         float* __restrict__ sout, float* __restrict__ ssm,
                                                         float* __restrict__ logits, int W, const float* __restrict__ params,
                                                         const SetLayer* __restrict__ layers, const SetTile* __restrict__ tiles) {
    const SetTile t = tiles[blockIdx.y];
    const SetLayer L = layers[t.layer];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tr = 2 * blockIdx.x + (wave & 1);         // 32-row tile of C
    const int tc = 2 * t.tile + (wave >> 1);            // 32-column tile of this layer
    if (32 * tr >= W || 32 * tc >= L.n) return;         // (no barrier in this kernel)
    const int half = lane >> 5;
    const int arow = min(32 * tr + (lane & 31), W - 1);
    const float* A = L.a_src == kFromPooled ? pooled : sin + L.a_col;
    const float* ap = A + (size_t)arow * L.lda + 4 * half;
    const float4* bp = reinterpret_cast<const float4*>(params + L.wf_off) + (size_t)tc * L.n_super * 64 + lane;

    const dense_v16f acc = dense_tile_walk(ap, bp, L.k, L.n_super, half);
    float* C = (L.c_dst == kToLogits ? logits : L.c_dst == kToScratch ? sout : ssm) + L.c_col;
    dense_tile_store(acc, params + L.bias_off, L.act, tr, tc, W, L.n, C, L.ldc, lane);
}

__global__ __launch_bounds__(256) void softmax_set_kernel(const float* __restrict__ ssm, float* __restrict__ logits, int ldy, int W,
                                                           const SetSoftmax* __restrict__ sm) {
    const int lane = threadIdx.x & 63;
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (row >= W) return;
    const SetSoftmax s = sm[blockIdx.y];
    softmax_row(ssm + (size_t)row * kHeadSetRow + s.x_col, logits + (size_t)row * ldy + s.y_col, s.n, lane);
}

__global__ __launch_bounds__(256) void head_set_kernel(const float* __restrict__ pooled, const float* __restrict__ head_wt,
                                                        const float* __restrict__ head_b, const int* __restrict__ col,
                                                        int n_fused, float* __restrict__ logits, int ldy) {
    // one workgroup per (window, group of <= 64 classes); pooled = [window][1024]
    __shared__ float s_part[4][BD_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const size_t win = blockIdx.x;
    const int g0 = BD_MAX_CLASSES * blockIdx.y;
    const int n_classes = min(BD_MAX_CLASSES, n_fused - g0);
    const float* wt = head_wt + (size_t)g0 * BD_EMBEDDING_SIZE;
    const float4 s = reinterpret_cast<const float4*>(pooled + win * BD_EMBEDDING_SIZE)[tid];
    for (int c0 = 0; c0 < n_classes; c0 += 16) {
        float4 w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j < n_classes ? c0 + j : n_classes - 1;
            w[j] = reinterpret_cast<const float4*>(wt + (size_t)c * BD_EMBEDDING_SIZE)[tid];
        }
        float p[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = fmaf(s.x, w[j].x, fmaf(s.y, w[j].y, fmaf(s.z, w[j].z, s.w * w[j].w)));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 16; ++j) p[j] += __shfl_xor(p[j], o, 64);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (lane == 0 && c0 + j < n_classes) s_part[wave][c0 + j] = p[j];
    }
    __syncthreads();
    if (tid < n_classes)
        logits[win * ldy + col[g0 + tid]] =
            ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) + head_b[g0 + tid];
}

inline int pad32(int v) { return (v + 31) / 32 * 32; }
inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

bool fused_route(const bd_headset_member& m, bool lone) {
    return !lone && m.n_layers == 1 && m.layers[0].activation == BD_HEAD_LINEAR && m.layers[0].n_out <= BD_MAX_CLASSES;
}

// The shape checks on one stack's layers; `stack` / `layer` open the messages ("bd_head_attach: " / "bd_head_attach: layer ")
int check_stack(const bd_head_layer* layers, int n_layers, const std::string& stack, const std::string& layer, std::string* err) {
    if (n_layers < 1 || n_layers > BD_HEAD_MAX_LAYERS) {
        *err = stack + "a stack has 1.." + std::to_string(BD_HEAD_MAX_LAYERS) + " layers, not " + std::to_string(n_layers);
        return BD_EINVAL;
    }
    int width = BD_EMBEDDING_SIZE;
    for (int i = 0; i < n_layers; ++i) {
        const bd_head_layer& L = layers[i];
        const std::string lw = layer + std::to_string(i);
        if (!L.kernel) { *err = lw + " has no kernel"; return BD_EINVAL; }
        if (L.n_out < 1 || L.n_out > BD_HEAD_MAX_WIDTH) {
            *err = lw + ": width " + std::to_string(L.n_out) + " outside 1.." + std::to_string(BD_HEAD_MAX_WIDTH);
            return BD_EINVAL;
        }
        if (L.n_in != width) {
            *err = lw + " takes " + std::to_string(L.n_in) + " inputs, the layer before it gives " + std::to_string(width);
            return BD_EINVAL;
        }
        if (L.activation < BD_HEAD_LINEAR || L.activation > BD_HEAD_SOFTMAX) {
            *err = lw + ": unknown activation " + std::to_string(L.activation);
            return BD_EINVAL;
        }
        if (L.activation == BD_HEAD_SOFTMAX && i + 1 != n_layers) { *err = lw + ": softmax on a hidden layer"; return BD_EINVAL; }
        width = L.n_out;
    }
    return BD_OK;
}

}  // namespace

int headset_build(const bd_headset_member* members, int n_members, bool lone, HeadSet* out, std::string* err) {
    const std::string fn = lone ? "bd_head_attach: " : "bd_headset_attach: ";
    if (n_members < 1 || n_members > BD_HEADSET_MAX_MEMBERS) {
        *err = fn + "a set has 1.." + std::to_string(BD_HEADSET_MAX_MEMBERS) + " members, not " + std::to_string(n_members);
        return BD_EINVAL;
    }
    int max_depth = 0;
    long long outputs = 0;
    for (int m = 0; m < n_members; ++m) {
        const bd_headset_member& M = members[m];
        const std::string who = fn + "member " + std::to_string(m);
        if (!M.layers) { *err = who + " has no layers"; return BD_EINVAL; }
        const int rc = lone ? check_stack(M.layers, M.n_layers, fn, fn + "layer ", err)
                            : check_stack(M.layers, M.n_layers, who + ": ", who + " layer ", err);
        if (rc != BD_OK) return rc;
        outputs += M.layers[M.n_layers - 1].n_out;
        if (!fused_route(M, lone) && M.n_layers > max_depth) max_depth = M.n_layers;
    }
    if (outputs > BD_HEAD_MAX_WIDTH) {
        *err = fn + "the members' outputs sum to " + std::to_string(outputs) + ", more than " + std::to_string(BD_HEAD_MAX_WIDTH);
        return BD_EINVAL;
    }
    for (int d = 0; d < max_depth; ++d) {
        long long sum = 0;
        for (int m = 0; m < n_members; ++m) {
            const bd_headset_member& M = members[m];
            if (fused_route(M, lone) || d >= M.n_layers) continue;
            if (d + 1 < M.n_layers || M.layers[d].activation == BD_HEAD_SOFTMAX) sum += pad32(M.layers[d].n_out);
        }
        if (sum > kHeadSetRow) {
            *err = fn + "depth " + std::to_string(d) + ": the hidden widths (each rounded up to 32) sum to " + std::to_string(sum) +
                   ", more than " + std::to_string(kHeadSetRow);
            return BD_EINVAL;
        }
    }

    // ---- layout: parameters (floats), then the descriptors ----
    HeadSet set;
    set.lone = lone;
    set.members = lone ? 0 : n_members;
    set.outputs = (int)outputs;
    std::vector<float> params;
    std::vector<std::vector<SetLayer>> layers(max_depth);
    std::vector<std::vector<SetTile>> tiles(max_depth);
    std::vector<SetSoftmax> softmax;
    std::vector<int> fused_col;
    std::vector<float> fused_wt, fused_b;
    std::vector<int> depth_at(max_depth, 0);              // next free column of the region depth d writes
    int col = 0, sm_col = 0;
    for (int m = 0; m < n_members; ++m) {
        const bd_headset_member& M = members[m];
        const int n_last = M.layers[M.n_layers - 1].n_out;
        set.first.push_back(col);
        set.count.push_back(n_last);
        set.last_act.push_back(M.layers[M.n_layers - 1].activation);
        if (fused_route(M, lone)) {
            const bd_head_layer& L = M.layers[0];
            for (int c = 0; c < L.n_out; ++c) {             // [1024][n] -> [class][1024], as bd_create keeps its head
                for (int k = 0; k < BD_EMBEDDING_SIZE; ++k) fused_wt.push_back(L.kernel[(size_t)k * L.n_out + c]);
                fused_b.push_back(L.bias ? L.bias[c] : 0.0f);
                fused_col.push_back(col + c);
            }
        } else {
            int a_col = 0;
            for (int d = 0; d < M.n_layers; ++d) {
                const bd_head_layer& L = M.layers[d];
                SetLayer D;
                std::memset(&D, 0, sizeof(D));
                D.a_src = d == 0 ? kFromPooled : kFromScratch;
                D.a_col = a_col;
                D.lda = d == 0 ? BD_EMBEDDING_SIZE : kHeadSetRow;
                D.k = L.n_in;
                D.n_super = pad32(L.n_in) / 8;
                D.n = L.n_out;
                D.act = L.activation;
                const bool last = d + 1 == M.n_layers;
                if (last && L.activation == BD_HEAD_SOFTMAX) {
                    D.c_dst = kToSoftmax; D.c_col = sm_col; D.ldc = kHeadSetRow;
                    softmax.push_back(SetSoftmax{sm_col, L.n_out, col});
                    sm_col += L.n_out;
                } else if (last) {
                    D.c_dst = kToLogits; D.c_col = col; D.ldc = set.outputs;
                } else {
                    D.c_dst = kToScratch; D.c_col = depth_at[d]; D.ldc = kHeadSetRow;
                    a_col = depth_at[d];
                    depth_at[d] += pad32(L.n_out);
                }
                D.wf_off = (long long)params.size();
                params.resize(params.size() + dense_packed_floats(L.n_in, L.n_out), 0.0f);
                dense_pack_weights(L.kernel, L.n_in, L.n_out, params.data() + D.wf_off);
                D.bias_off = (int)params.size();
                params.resize(params.size() + (size_t)(L.n_out + 3) / 4 * 4, 0.0f);
                if (L.bias) std::memcpy(params.data() + D.bias_off, L.bias, (size_t)L.n_out * sizeof(float));
                if (params.size() >= (1u << 30)) { *err = fn + "the members' kernels exceed 4 GB"; return BD_EINVAL; }
                for (int t = 0; t < (L.n_out + 63) / 64; ++t) tiles[d].push_back(SetTile{(int)layers[d].size(), t});
                layers[d].push_back(D);
            }
        }
        col += n_last;
    }
    set.n_softmax = (int)softmax.size();
    set.n_fused = (int)fused_col.size();

    // one allocation: [params][fused_wt][fused_b][fused_col][per depth: layers, tiles][softmax], each part 16-byte aligned
    size_t at = 0;
    auto reserve = [&](size_t bytes) { const size_t o = at; at = up16(at + bytes); return o; };
    const size_t o_params = reserve(params.size() * 4), o_fwt = reserve(fused_wt.size() * 4), o_fb = reserve(fused_b.size() * 4),
                 o_fcol = reserve(fused_col.size() * 4);
    std::vector<size_t> o_layers, o_tiles;
    for (int d = 0; d < max_depth; ++d) {
        o_layers.push_back(reserve(layers[d].size() * sizeof(SetLayer)));
        o_tiles.push_back(reserve(tiles[d].size() * sizeof(SetTile)));
    }
    const size_t o_sm = reserve(softmax.size() * sizeof(SetSoftmax));
    std::vector<char> host(at + 16, 0);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(host.data() + o, src, bytes); };
    put(o_params, params.data(), params.size() * 4);
    put(o_fwt, fused_wt.data(), fused_wt.size() * 4);
    put(o_fb, fused_b.data(), fused_b.size() * 4);
    put(o_fcol, fused_col.data(), fused_col.size() * 4);
    for (int d = 0; d < max_depth; ++d) {
        put(o_layers[d], layers[d].data(), layers[d].size() * sizeof(SetLayer));
        put(o_tiles[d], tiles[d].data(), tiles[d].size() * sizeof(SetTile));
    }
    put(o_sm, softmax.data(), softmax.size() * sizeof(SetSoftmax));
    char* dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&dev), host.size()) != hipSuccess) { *err = fn + "hipMalloc failed"; return BD_EHIP; }
    if (hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        *err = fn + "upload failed";
        return BD_EHIP;
    }
    set.dev = dev;
    for (int d = 0; d < max_depth; ++d) set.depths.push_back(HeadSet::Depth{dev + o_layers[d], dev + o_tiles[d], (int)tiles[d].size()});
    set.softmax = dev + o_sm;
    set.fused_wt = reinterpret_cast<const float*>(dev + o_fwt);
    set.fused_b = reinterpret_cast<const float*>(dev + o_fb);
    set.fused_col = reinterpret_cast<const int*>(dev + o_fcol);
    *out = std::move(set);
    return BD_OK;
}

void headset_free(HeadSet* set) {
    if (set->dev) (void)hipFree(set->dev);
    *set = HeadSet();
}

void launch_dense_set(const HeadSet& set, int depth, const float* pooled, float* scratch, float* logits, int windows,
                      hipStream_t stream) {
    const HeadSet::Depth& D = set.depths[depth];
    if (windows <= 0 || D.n_tiles == 0) return;
    const size_t region = (size_t)windows * kHeadSetRow;
    hipLaunchKernelGGL(dense_set_kernel, dim3((windows + 63) / 64, D.n_tiles), dim3(256), 0, stream, pooled,
                       scratch + ((depth + 1) & 1) * region, scratch + (depth & 1) * region, scratch + 2 * region, logits, windows,
                       reinterpret_cast<const float*>(set.dev), static_cast<const SetLayer*>(D.layers),
                       static_cast<const SetTile*>(D.tiles));
}

void launch_softmax_set(const HeadSet& set, const float* scratch, float* logits, int windows, hipStream_t stream) {
    if (windows <= 0 || set.n_softmax == 0) return;
    hipLaunchKernelGGL(softmax_set_kernel, dim3((windows + 3) / 4, set.n_softmax), dim3(256), 0, stream,
                       scratch + 2 * (size_t)windows * kHeadSetRow, logits, set.outputs, windows,
                       static_cast<const SetSoftmax*>(set.softmax));
}

void launch_head_set(const HeadSet& set, const float* pooled, float* logits, int windows, hipStream_t stream) {
    if (windows <= 0 || set.n_fused == 0) return;
    hipLaunchKernelGGL(head_set_kernel, dim3(windows, (set.n_fused + BD_MAX_CLASSES - 1) / BD_MAX_CLASSES), dim3(256), 0, stream,
                       pooled, set.fused_wt, set.fused_b, set.fused_col, set.n_fused, logits, set.outputs);
}

}  // namespace bd

extern "C" {

int bd_headset_abi_version(void) { return BD_HEADSET_ABI_VERSION; }

int bd_headset_members(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_headset_members: null handle");
    return h->set.members;
}

int bd_headset_outputs(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_headset_outputs: null handle");
    return h->set.lone ? 0 : h->set.outputs;
}

int bd_headset_columns(bd_handle h, int32_t member, int32_t* first, int32_t* count) {
    if (!h || !first || !count) return fail(BD_EINVAL, "bd_headset_columns: null argument");
    if (member < 0 || member >= h->set.members)
        return fail(BD_EINVAL, "bd_headset_columns: member " + std::to_string(member) + " outside 0.." +
                                   std::to_string(h->set.members - 1));
    *first = h->set.first[member];
    *count = h->set.count[member];
    return BD_OK;
}

int bd_headset_attach(bd_handle h, const bd_headset_member* members, int32_t n_members) {
    if (!h || !members) return fail(BD_EINVAL, "bd_headset_attach: null argument");
    if (h->set.members) return fail(BD_EINVAL, "bd_headset_attach: the engine already has a set of heads");
    if (h->set.lone) return fail(BD_EINVAL, "bd_headset_attach: the engine already has a stack (bd_head_attach)");
    if (h->n_classes != 0)
        return fail(BD_EINVAL, "bd_headset_attach: the engine already has a head (create it with n_classes == 0)");
    BD_HIP(hipSetDevice(h->device));
    std::string err;
    bd::HeadSet set;
    const int rc = bd::headset_build(members, n_members, false, &set, &err);
    if (rc != BD_OK) return fail(rc, err);
    h->set = std::move(set);
    h->n_classes = h->set.outputs;
    return BD_OK;
}

}  // extern "C"
