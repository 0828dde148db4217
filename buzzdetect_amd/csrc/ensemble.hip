// Ensembles of heads (include/buzzdetect_ensemble.h): the members of an attached set (headset.hip) reduced to one output per
// group, on the device, in ONE launch per pass whatever the number of members.
//
//   ensemble_combine_kernel   grid (4 windows, output), a wave per (window, output).  The set's launches have left the members'
//                             columns in a scratch row packed like the logits they would otherwise have written (bd_internal.h:
//                             region kEnsembleRegion); the members of one output are contiguous there and share a width.  Lanes
//                             stride the output's columns in ascending order; a column is computed by one lane alone, with the
//                             routines of ensemble_device.h - the text bd_ensemble_combine_host below calls too.  A pass-through
//                             output is copied.  Only the soft vote over softmax needs anything across a row: each member's
//                             log-sum-exp, reduced over the wave with xor butterflies as softmax_row does (dense_device.h) and
//                             parked in LDS, one slot per member.
//
// Nothing is added atomically, nothing is split over workgroups, the wide row is only read: the launch is idempotent and
// bit-reproducible.
#include "engine_state.h"
#include "ensemble_device.h"

#include <cstring>

#include "../../include/buzzdetect_ensemble.h"

namespace bd {
namespace {

struct EnsOutput {
    int wide_col, k, width, out_col;     // member 0's first column of the wide row, members, their common width, first public column
    int combine, link;
    float r, log_k;                      // 1.0f / k and logf(k), rounded once on the host
};

__global__ __launch_bounds__(256) void ensemble_combine_kernel(const float* __restrict__ wide, int ld_wide, float* __restrict__ logits,
                                                                int ld_out, int W, const EnsOutput* __restrict__ outs) {
    __shared__ float s_lse[4][BD_HEADSET_MAX_MEMBERS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int row = 4 * blockIdx.x + wave;
    const bool live = row < W;                                // a wave past the last window reads the last row and writes nothing
    const size_t r = (size_t)(live ? row : W - 1);
    const EnsOutput o = outs[blockIdx.y];
    const float* __restrict__ z = wide + r * ld_wide + o.wide_col;
    float* __restrict__ y = logits + r * ld_out + o.out_col;
    const int n = o.width;
    if (o.combine == BD_COMBINE_MEAN_PROBABILITY && o.link == BD_LINK_SOFTMAX) {       // (uniform over the workgroup)
        for (int m = 0; m < o.k; ++m) {
            const float* __restrict__ p = z + (size_t)m * n;
            float mx = -INFINITY;
            for (int c = lane; c < n; c += 64) mx = fmaxf(mx, p[c]);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            float sum = 0.0f;
            for (int c = lane; c < n; c += 64) sum += expf(p[c] - mx);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
            if (lane == 0) s_lse[wave][m] = ens::lse_of(mx, sum);
        }
        __syncthreads();
        if (live)
            for (int c = lane; c < n; c += 64) y[c] = ens::mean_probability_softmax(z + c, n, s_lse[wave], o.k, o.log_k);
    } else if (!live) {
        return;
    } else if (o.combine == BD_COMBINE_MEAN_PROBABILITY) {
        for (int c = lane; c < n; c += 64) y[c] = ens::mean_probability_sigmoid(z + c, n, o.k);
    } else if (o.combine == BD_COMBINE_MEAN) {
        for (int c = lane; c < n; c += 64) y[c] = ens::mean(z + c, n, o.k, o.r);
    } else {
        for (int c = lane; c < n; c += 64) y[c] = z[c];
    }
}

// what attach and the host restatement both refuse about the outputs themselves; width[m]: member m's last width
int check_outputs(const std::string& fn, const bd_ensemble_output* outputs, int n_outputs, int n_members, const int* width,
                  std::string* err) {
    if (n_outputs < 1 || n_outputs > BD_HEADSET_MAX_MEMBERS) {
        *err = fn + "an ensemble has 1.." + std::to_string(BD_HEADSET_MAX_MEMBERS) + " outputs, not " + std::to_string(n_outputs);
        return BD_EINVAL;
    }
    int at = 0;
    for (int o = 0; o < n_outputs; ++o) {
        const bd_ensemble_output& O = outputs[o];
        const std::string who = fn + "output " + std::to_string(o);
        if (O.n_members < 1) { *err = who + " has " + std::to_string(O.n_members) + " members, at least 1 is needed"; return BD_EINVAL; }
        if (O.first_member != at) {
            *err = who + " starts at member " + std::to_string(O.first_member) + ", the outputs before it end at member " +
                   std::to_string(at) + " (outputs tile the set's members in order, without gap or overlap)";
            return BD_EINVAL;
        }
        if (O.n_members > n_members - at) {
            *err = who + " takes members " + std::to_string(at) + ".." + std::to_string(at + O.n_members - 1) + ", the set has " +
                   std::to_string(n_members);
            return BD_EINVAL;
        }
        if (O.combine < BD_COMBINE_NONE || O.combine > BD_COMBINE_MEAN_PROBABILITY) {
            *err = who + ": unknown combine " + std::to_string(O.combine);
            return BD_EINVAL;
        }
        if (O.link < BD_LINK_NONE || O.link > BD_LINK_SIGMOID) { *err = who + ": unknown link " + std::to_string(O.link); return BD_EINVAL; }
        if (O.combine == BD_COMBINE_NONE && O.n_members != 1) {
            *err = who + ": BD_COMBINE_NONE passes one member through, not " + std::to_string(O.n_members);
            return BD_EINVAL;
        }
        if (O.combine == BD_COMBINE_MEAN_PROBABILITY && O.link == BD_LINK_NONE) {
            *err = who + ": BD_COMBINE_MEAN_PROBABILITY needs a link (BD_LINK_SOFTMAX or BD_LINK_SIGMOID)";
            return BD_EINVAL;
        }
        if (O.combine != BD_COMBINE_MEAN_PROBABILITY && O.link != BD_LINK_NONE) {
            *err = who + ": a link goes with BD_COMBINE_MEAN_PROBABILITY only";
            return BD_EINVAL;
        }
        for (int m = at + 1; m < at + O.n_members; ++m) {
            if (width[m] != width[at]) {
                *err = who + ": member " + std::to_string(m) + " gives " + std::to_string(width[m]) + " outputs, member " +
                       std::to_string(at) + " gives " + std::to_string(width[at]);
                return BD_EINVAL;
            }
        }
        at += O.n_members;
    }
    if (at != n_members) {
        *err = fn + "the outputs cover members 0.." + std::to_string(at - 1) + ", the set has " + std::to_string(n_members);
        return BD_EINVAL;
    }
    return BD_OK;
}

EnsOutput describe(const bd_ensemble_output& O, int wide_col, int width, int out_col) {
    EnsOutput D;
    std::memset(&D, 0, sizeof(D));
    D.wide_col = wide_col;
    D.k = O.n_members;
    D.width = width;
    D.out_col = out_col;
    D.combine = O.combine;
    D.link = O.link;
    D.r = 1.0f / (float)O.n_members;
    D.log_k = logf((float)O.n_members);
    return D;
}

}  // namespace

int ensemble_build(const HeadSet& set, const bd_ensemble_output* outputs, int n_outputs, Ensemble* out, std::string* err) {
    const std::string fn = "bd_ensemble_attach: ";
    const int rc = check_outputs(fn, outputs, n_outputs, set.members, set.count.data(), err);
    if (rc != BD_OK) return rc;
    Ensemble ens;
    std::vector<EnsOutput> desc;
    int col = 0;
    for (int o = 0; o < n_outputs; ++o) {
        const bd_ensemble_output& O = outputs[o];
        const std::string who = fn + "output " + std::to_string(o);
        const int m0 = O.first_member;
        for (int m = m0 + 1; m < m0 + O.n_members; ++m) {
            if (set.last_act[m] != set.last_act[m0]) {
                *err = who + ": member " + std::to_string(m) + " ends in activation " + std::to_string(set.last_act[m]) + ", member " +
                       std::to_string(m0) + " in " + std::to_string(set.last_act[m0]);
                return BD_EINVAL;
            }
        }
        if (O.combine == BD_COMBINE_MEAN_PROBABILITY && set.last_act[m0] != BD_HEAD_LINEAR) {
            *err = who + ": BD_COMBINE_MEAN_PROBABILITY takes members whose last layer is linear; member " + std::to_string(m0) +
                   " ends in activation " + std::to_string(set.last_act[m0]);
            return BD_EINVAL;
        }
        desc.push_back(describe(O, set.first[m0], set.count[m0], col));
        ens.first.push_back(col);
        ens.count.push_back(set.count[m0]);
        col += set.count[m0];
    }
    ens.n_outputs = n_outputs;
    ens.columns = col;
    if (hipMalloc(&ens.dev, desc.size() * sizeof(EnsOutput)) != hipSuccess) { *err = fn + "hipMalloc failed"; return BD_EHIP; }
    if (hipMemcpy(ens.dev, desc.data(), desc.size() * sizeof(EnsOutput), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(ens.dev);
        *err = fn + "upload failed";
        return BD_EHIP;
    }
    *out = std::move(ens);
    return BD_OK;
}

void ensemble_free(Ensemble* ens) {
    if (ens->dev) (void)hipFree(ens->dev);
    *ens = Ensemble();
}

void launch_ensemble_combine(const Ensemble& ens, const float* wide, int ld_wide, float* logits, int windows, hipStream_t stream) {
    if (windows <= 0 || ens.n_outputs == 0) return;
    hipLaunchKernelGGL(ensemble_combine_kernel, dim3((windows + 3) / 4, ens.n_outputs), dim3(256), 0, stream, wide, ld_wide, logits,
                       ens.columns, windows, static_cast<const EnsOutput*>(ens.dev));
}

}  // namespace bd

extern "C" {

int bd_ensemble_abi_version(void) { return BD_ENSEMBLE_ABI_VERSION; }

int bd_ensemble_count(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_ensemble_count: null handle");
    return h->ens.n_outputs;
}

int bd_ensemble_outputs(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_ensemble_outputs: null handle");
    return h->ens.columns;
}

int bd_ensemble_columns(bd_handle h, int32_t output, int32_t* first, int32_t* count) {
    if (!h || !first || !count) return fail(BD_EINVAL, "bd_ensemble_columns: null argument");
    if (output < 0 || output >= h->ens.n_outputs)
        return fail(BD_EINVAL, "bd_ensemble_columns: output " + std::to_string(output) + " outside 0.." +
                                   std::to_string(h->ens.n_outputs - 1));
    *first = h->ens.first[output];
    *count = h->ens.count[output];
    return BD_OK;
}

int bd_ensemble_attach(bd_handle h, const bd_ensemble_output* outputs, int32_t n_outputs) {
    if (!h || !outputs) return fail(BD_EINVAL, "bd_ensemble_attach: null argument");
    if (!h->set.members) return fail(BD_EINVAL, "bd_ensemble_attach: the engine has no set of heads (bd_headset_attach comes first)");
    if (h->ens.n_outputs) return fail(BD_EINVAL, "bd_ensemble_attach: the engine already has an ensemble");
    BD_HIP(hipSetDevice(h->device));
    std::string err;
    bd::Ensemble ens;
    const int rc = bd::ensemble_build(h->set, outputs, n_outputs, &ens, &err);
    if (rc != BD_OK) return fail(rc, err);
    h->ens = std::move(ens);
    h->n_classes = h->ens.columns;
    return BD_OK;
}

int bd_ensemble_combine_host(const float* wide, int64_t windows, int32_t ld_wide, const bd_ensemble_output* outputs, int32_t n_outputs,
                             const int32_t* member_first, float* out, int32_t ld_out) {
    const std::string fn = "bd_ensemble_combine_host: ";
    if (!outputs || !member_first || windows < 0 || (windows > 0 && (!wide || !out))) {
        bd::set_error(fn + "null argument or a negative number of windows");
        return BD_EINVAL;
    }
    int n_members = 0;
    for (int o = 0; o < n_outputs; ++o) {
        if (outputs[o].n_members < 1) {
            bd::set_error(fn + "output " + std::to_string(o) + " has " + std::to_string(outputs[o].n_members) +
                          " members, at least 1 is needed");
            return BD_EINVAL;
        }
        if (outputs[o].n_members > BD_HEADSET_MAX_MEMBERS - n_members) { n_members = -1; break; }
        n_members += outputs[o].n_members;
    }
    if (n_outputs < 1 || n_members < 1) {
        bd::set_error(fn + "the outputs name 1.." + std::to_string(BD_HEADSET_MAX_MEMBERS) + " members in all, not " +
                      (n_outputs < 1 ? std::string("none") : std::string("more")));
        return BD_EINVAL;
    }
    std::vector<int> width(n_members);
    for (int m = 0; m < n_members; ++m) {
        width[m] = member_first[m + 1] - member_first[m];
        if (member_first[m] < 0 || width[m] < 1 || member_first[m + 1] > ld_wide) {
            bd::set_error(fn + "member " + std::to_string(m) + " takes columns " + std::to_string(member_first[m]) + ".." +
                          std::to_string(member_first[m + 1]) + " of " + std::to_string(ld_wide));
            return BD_EINVAL;
        }
    }
    std::string err;
    const int rc = bd::check_outputs(fn, outputs, n_outputs, n_members, width.data(), &err);
    if (rc != BD_OK) {
        bd::set_error(err);
        return rc;
    }
    std::vector<bd::EnsOutput> desc;
    int col = 0;
    for (int o = 0; o < n_outputs; ++o) {
        const int m0 = outputs[o].first_member;
        desc.push_back(bd::describe(outputs[o], member_first[m0], width[m0], col));
        col += width[m0];
    }
    if (col > ld_out) {
        bd::set_error(fn + "the outputs take " + std::to_string(col) + " columns, ld_out is " + std::to_string(ld_out));
        return BD_EINVAL;
    }
    float lse[BD_HEADSET_MAX_MEMBERS];
    for (int64_t w = 0; w < windows; ++w) {
        for (const bd::EnsOutput& o : desc) {
            const float* z = wide + (size_t)w * ld_wide + o.wide_col;
            float* y = out + (size_t)w * ld_out + o.out_col;
            const int n = o.width;
            if (o.combine == BD_COMBINE_MEAN_PROBABILITY && o.link == BD_LINK_SOFTMAX) {
                for (int m = 0; m < o.k; ++m) {
                    const float* p = z + (size_t)m * n;
                    float mx = -INFINITY;
                    for (int c = 0; c < n; ++c) mx = fmaxf(mx, p[c]);
                    float sum = 0.0f;
                    for (int c = 0; c < n; ++c) sum += expf(p[c] - mx);
                    lse[m] = bd::ens::lse_of(mx, sum);
                }
                for (int c = 0; c < n; ++c) y[c] = bd::ens::mean_probability_softmax(z + c, n, lse, o.k, o.log_k);
            } else if (o.combine == BD_COMBINE_MEAN_PROBABILITY) {
                for (int c = 0; c < n; ++c) y[c] = bd::ens::mean_probability_sigmoid(z + c, n, o.k);
            } else if (o.combine == BD_COMBINE_MEAN) {
                for (int c = 0; c < n; ++c) y[c] = bd::ens::mean(z + c, n, o.k, o.r);
            } else {
                for (int c = 0; c < n; ++c) y[c] = z[c];
            }
        }
    }
    return BD_OK;
}

}  // extern "C"
