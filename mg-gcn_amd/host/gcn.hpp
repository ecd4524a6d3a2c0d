// gcn.hpp -- the layer API of the reference (src/gcn.hpp) over the HIP engine.
//
// sparse_linear (:13-48), dist_sparse_linear (:50-86), linear (:88-189), dist_row_linear
// (:191-296), gcn_layer (:411-518), dist_gcn_layer (:520-637), softmax (:639-676),
// softmax_cross_entropy_loss (:769-823), dist_row_softmax_cross_entropy_loss (:872-935),
// gcn (:937-995), dist_gcn (:997-1056): same names, constructor arguments, members, buffer
// aliasing (model-wide HW_buffer; per-layer AHW_buffer holding AHW forward / G_out backward),
// layer-order rule (out <= in: GEMM first), skipped first-layer backward SpMM, timer names.
// `fused` (default on in gcn / dist_gcn) folds leaky-ReLU into the SpMM epilogue and uses the
// one-pass loss and one-launch Adam kernels; fused = false replays the reference's launches.
#pragma once

#include <array>
#include <cmath>
#include <limits>
#include <numeric>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "checkpoint.hpp"
#include "dist_matrix.hpp"
#include "matrix.hpp"
#include "ops.hpp"

// Storage of the gathered operand of the model's SpMMs: f32 (the reference's), or bf16 -- every aggregation rounds its
// dense input to bf16 into one model-owned scratch and multiplies with mggcn_spmm_csr_bf16 (sums and all else fp32).
enum class agg_dtype { f32, bf16 };

inline agg_dtype agg_dtype_from_string(const std::string &s) {
    if (s.empty() || s == "f32") return agg_dtype::f32;
    if (s == "bf16") return agg_dtype::bf16;
    throw std::invalid_argument("aggregation dtype must be f32 or bf16, not '" + s + "'");
}

template <typename x_t, typename v_t, typename r_t>
class sparse_linear {
    using csr_t = csr_matrix<x_t, v_t, r_t>;
    using dn_t = dn_matrix<r_t>;
    std::string name;
    csr_t A, A_T;
    spmm_buffer ext_buffer, ext_buffer2;
    agg_dtype agg;
    mggcn::device_ptr<std::uint16_t> agg_buffer;     // bf16: the rounded dense operand (shared by the model's layers)
    std::size_t agg_capacity;

    void spmm(context ctx, const csr_t &M, dn_t B, dn_t C, const spmm_buffer &plan, r_t beta, uint32_t flags) {
        if (agg == agg_dtype::f32) { matmul(ctx, M, B, C, plan, (r_t)1, beta, flags); return; }
        if (!agg_buffer || agg_capacity < B.n() * B.m()) {
            agg_capacity = B.n() * B.m();
            agg_buffer = mggcn::device_malloc<std::uint16_t>(agg_capacity);
        }
        convert_bf16(ctx, B, agg_buffer.get(), B.m());
        matmul_bf16(ctx, M, agg_buffer.get(), B.m(), C, plan, (r_t)1, beta, flags);
    }

public:
    sparse_linear(std::string name, csr_t A, csr_t A_T, agg_dtype agg = agg_dtype::f32,
                  mggcn::device_ptr<std::uint16_t> agg_buffer = nullptr, std::size_t agg_capacity = 0)
        : name(name), A(A), A_T(A_T), agg(agg), agg_buffer(agg_buffer), agg_capacity(agg_buffer ? agg_capacity : 0) {}
    const csr_t &forward_matrix() const { return A; }

    void operator()(context ctx, dn_t B, dn_t C, bool discard = true, uint32_t flags = 0) {
        if (!ext_buffer) ext_buffer = get_matmul_buffer(ctx, A, B, C);      // plan is width-independent up to 128+
        ctx.record(name + "0_0_matmul-spmm", 0);
        spmm(ctx, A, B, C, ext_buffer, discard ? (r_t)0 : (r_t)1, flags);
        ctx.record(name + "0_1_matmul-spmm", 0);
        ctx.register_timer(name + "0_matmul-spmm", name + "0_0_matmul-spmm", name + "0_1_matmul-spmm");
    }

    void backward(context ctx, dn_t G, dn_t G_out, bool discard = true) {
        if (!ext_buffer2) ext_buffer2 = get_matmul_buffer(ctx, A_T, G, G_out);
        ctx.record(name + "1_0_matmul-spmm", 0);
        spmm(ctx, A_T, G, G_out, ext_buffer2, discard ? (r_t)0 : (r_t)1, 0);
        ctx.record(name + "1_1_matmul-spmm", 0);
        ctx.register_timer(name + "1_matmul-spmm", name + "1_0_matmul-spmm", name + "1_1_matmul-spmm");
    }
};

template <bool row_partition, typename x_t, typename v_t, typename r_t>
class dist_sparse_linear {
    static_assert(row_partition, "only the row partition is live in the reference CLI");
    using csr_t = dist_row_csr_matrix<x_t, v_t, r_t>;
    using dn_t = dist_row_dn_matrix<r_t>;
    std::string name;
    csr_t A, A_T;
    std::vector<mggcn::device_ptr<r_t>> bcast_buffer, bcast_buffer2;
    dist_mode mode;
    dist_spmm_buffers ext, ext2;
    std::size_t M = 0, M2 = 0;                     // width the buffers were built for (reference :28-31)
    std::shared_ptr<dist_halo_plan<r_t>> halo, halo2;

    // receive buffers as matrices of the current width
    std::vector<dn_t> round_views(const dist_context &ctx, const dn_t &B) const {
        return {dn_t(ctx, B.n(), B.m(), bcast_buffer), dn_t(ctx, B.n(), B.m(), bcast_buffer2)};
    }
    std::vector<dn_matrix<r_t>> gather_views(const dist_context &ctx, const dn_t &B) const {
        std::vector<dn_matrix<r_t>> g;
        for (std::size_t j = 0; j < ctx.size(); j++) g.emplace_back(B.n(), B.m(), bcast_buffer[j]);
        return g;
    }

    void run(const dist_context &ctx, const csr_t &Mx, dn_t B, dn_t C, dist_spmm_buffers &e, std::size_t &width,
             std::shared_ptr<dist_halo_plan<r_t>> &hp, r_t beta, const std::string &tag, uint32_t flags) {
        if (width != B.m()) { e = get_matmul_buffer(ctx, Mx, B, C, mode); width = B.m(); }
        switch (mode) {
            case dist_mode::rounds: matmul(ctx, Mx, B, C, e, round_views(ctx, B), (r_t)1, beta, name + tag, flags); break;
            case dist_mode::allgather: matmul_allgather(ctx, Mx, B, C, e, gather_views(ctx, B), (r_t)1, beta, name + tag, flags); break;
            case dist_mode::halo:
                if (!hp) { ctx.drain(); hp = std::make_shared<dist_halo_plan<r_t>>(ctx, Mx); }
                matmul_halo(ctx, Mx, B, C, e, *hp, gather_views(ctx, B), (r_t)1, beta, name + tag, flags);
                break;
        }
    }

public:
    dist_sparse_linear(std::string name, csr_t A, csr_t A_T, std::vector<mggcn::device_ptr<r_t>> bcast_buffer,
                       std::vector<mggcn::device_ptr<r_t>> bcast_buffer2, dist_mode mode = dist_mode::allgather)
        : name(name), A(A), A_T(A_T), bcast_buffer(bcast_buffer), bcast_buffer2(bcast_buffer2), mode(mode) {}

    void operator()(const dist_context ctx, dn_t B, dn_t C, bool discard = true, uint32_t flags = 0) {
        run(ctx, A, B, C, ext, M, halo, discard ? (r_t)0 : (r_t)1, "0_", flags);
    }

    void backward(const dist_context ctx, dn_t G, dn_t G_out, bool discard = true) {
        run(ctx, A_T, G, G_out, ext2, M2, halo2, discard ? (r_t)0 : (r_t)1, "1_", 0u);
    }
};

// Adam step of one GPU's parameters (reference src/gcn.hpp:146-172)
template <typename r_t>
void adam_step(context ctx, bool fused, dn_matrix<r_t> W, dn_matrix<r_t> G_W, dn_matrix<r_t> mW, dn_matrix<r_t> vW, dn_matrix<r_t> b,
               dn_matrix<r_t> G_b, dn_matrix<r_t> mb, dn_matrix<r_t> vb, r_t lr, r_t beta1, r_t beta2, r_t wd, r_t eps, std::size_t step) {
    const r_t bc1 = 1 - std::pow(beta1, step);
    const r_t bc2 = 1 - std::pow(beta2, step);
    if (fused) {
        adam_fused(ctx, W, G_W, mW, vW, lr, beta1, beta2, wd, bc1, bc2, eps);
        adam_fused(ctx, b, G_b, mb, vb, lr, beta1, beta2, (r_t)0, bc1, bc2, eps);
        return;
    }
    axpy(ctx, W, G_W, wd);
    axpby(ctx, G_W, mW, 1 - beta1, beta1);
    axpby(ctx, G_b, mb, 1 - beta1, beta1);
    aaxpby(ctx, G_W, vW, 1 - beta2, beta2);
    aaxpby(ctx, G_b, vb, 1 - beta2, beta2);
    adam_final(ctx, W, mW, vW, lr, bc1, bc2, eps);
    adam_final(ctx, b, mb, vb, lr, bc1, bc2, eps);
}
template <typename r_t>
void adam_step(dist_context ctx, bool fused, repl_dn_matrix<r_t> W, repl_dn_matrix<r_t> G_W, repl_dn_matrix<r_t> mW, repl_dn_matrix<r_t> vW,
               repl_dn_matrix<r_t> b, repl_dn_matrix<r_t> G_b, repl_dn_matrix<r_t> mb, repl_dn_matrix<r_t> vb, r_t lr, r_t beta1, r_t beta2,
               r_t wd, r_t eps, std::size_t step) {
    for (std::size_t i = 0; i < ctx.size(); i++)
        ctx.on(i, [c = ctx[i], fused, w = W[i], gw = G_W[i], mw = mW[i], vw = vW[i], bb = b[i], gb = G_b[i], m_b = mb[i], v_b = vb[i],
                   lr, beta1, beta2, wd, eps, step] { adam_step(c, fused, w, gw, mw, vw, bb, gb, m_b, v_b, lr, beta1, beta2, wd, eps, step); });
}

// the row of ones of the reference's G_b GEMM (host-filled, :127-128), as long as one GPU's rows of G
template <typename r_t>
void ones_row(const context &, dn_matrix<r_t> &ones, const dn_matrix<r_t> &G) {
    if (ones.n() != 1 || ones.m() != G.n()) { ones = dn_matrix<r_t>(1, G.n()); ones.fill(1); }
}
template <typename r_t>
void ones_row(const dist_context &ctx, repl_dn_matrix<r_t> &ones, const dist_row_dn_matrix<r_t> &G) {
    const std::size_t rows = G.n() / ctx.size();
    if (ones.size() != ctx.size() || ones.m() != rows) { ctx.drain(); ones = repl_dn_matrix<r_t>(ctx, 1, rows); ones.fill(ctx, 1); }
}

template <typename r_t>
dn_matrix<r_t> zeros_like(const context &ctx, const dn_matrix<r_t> &A) {
    dn_matrix<r_t> z(A.shape());
    z.zero(ctx);
    return z;
}
template <typename r_t>
repl_dn_matrix<r_t> zeros_like(const dist_context &ctx, const repl_dn_matrix<r_t> &A) {
    repl_dn_matrix<r_t> z(ctx, A.shape());
    z.zero(ctx);
    return z;
}

// One linear layer (reference :88-189 / :191-296), written once over the context and matrix types: one GPU
// (context; rows and parameters dn_matrix) or the row partition (dist_context; rows dist_row_dn_matrix, parameters
// repl_dn_matrix), whose per-GPU loops come from the dist_context overloads.  What the row partition adds lives in the two
// hooks it overrides: reduce_gradients (after the weight-gradient GEMMs) and finish_backward.
template <typename r_t, typename ctx_t, template <typename> class dn_t, template <typename> class rdn_t>
class linear_body {
protected:
    std::string name;
    rdn_t<r_t> W, G_W, mW, vW, b, G_b, mb, vb, ones;
    dn_t<r_t> X;
    bool backward_out, fused, has_moments = false;
    std::size_t step = 0;

    linear_body(std::string name, rdn_t<r_t> W, rdn_t<r_t> G_W, rdn_t<r_t> b, rdn_t<r_t> G_b, bool backward_out, bool fused)
        : name(name), W(W), G_W(G_W), b(b), G_b(G_b), backward_out(backward_out), fused(fused) {}
    virtual void reduce_gradients(const ctx_t &) {}

public:
    // the compute stream sees the final gradients from here on
    virtual void finish_backward(const ctx_t &) {}

    void setX(dn_t<r_t> new_X) { X = new_X; }

    void operator()(ctx_t ctx, dn_t<r_t> X, dn_t<r_t> XW, bool discard = true) {
        if (fused && discard) {                      // bias in the GEMM epilogue
            ctx.record(name + "0_0_matmul-gemm", 0);
            linear_forward(ctx, X, W, b, XW);
        } else {
            broadcast_rows(ctx, b, XW, discard);
            ctx.record(name + "0_0_matmul-gemm", 0);
            matmul(ctx, X, W, XW, (r_t)1, (r_t)1);
        }
        ctx.record(name + "0_1_matmul-gemm", 0);
        ctx.register_timer(name + "0_matmul-gemm", name + "0_0_matmul-gemm", name + "0_1_matmul-gemm");
        this->X = X;
    }

    // mask (fused path): the activated output Z of the layer below; G_out leaves the GEMM already multiplied by
    // leaky_relu'(Z), i.e. it IS that layer's T (reference :462-468)
    void backward(ctx_t ctx, dn_t<r_t> G, dn_t<r_t> G_out, bool discard = true, const dn_t<r_t> *mask = nullptr) {
        if (!fused) ones_row(ctx, ones, G);
        ctx.record(name + "1_0_matmul-gemm", 0);
        linear_weight_gradients(ctx, fused, ones, X, G, G_W, G_b);
        reduce_gradients(ctx);
        ctx.record(name + "1_2_matmul-gemm", 0);
        if (backward_out && mask) matmul_lrelu_backward(ctx, G, W, *mask, G_out, (r_t)1, false, true);
        else if (backward_out) matmul(ctx, G, W, G_out, (r_t)1, discard ? (r_t)0 : (r_t)1, false, true);
        ctx.record(name + "1_3_matmul-gemm", 0);
        ctx.register_timer(name + "1_matmul-gemm", name + "1_0_matmul-gemm", name + "1_3_matmul-gemm");
    }

    void update(const ctx_t ctx, const r_t lr, const r_t weight_decay) {
        axpby(ctx, G_W, W, -lr, 1 - weight_decay);
        axpy(ctx, G_b, b, -lr);
    }

    bool has_backward_out() const { return backward_out; }

    // Adam moments, zeroed on first use; bump_step() for the model-wide single launch (gcn::adam_update)
    void adam_state(ctx_t ctx) {
        if (has_moments) return;
        mW = zeros_like(ctx, W); vW = zeros_like(ctx, W); mb = zeros_like(ctx, b); vb = zeros_like(ctx, b);
        has_moments = true;
        step = 0;
    }
    std::size_t bump_step() { return ++step; }

    void adam_update(ctx_t ctx, const r_t lr, const r_t beta1, const r_t beta2, const r_t weight_decay, const r_t eps) {
        finish_backward(ctx);
        adam_state(ctx);
        step += 1;
        ctx.record(name + "0_adam-update", 0);
        adam_step(ctx, fused, W, G_W, mW, vW, b, G_b, mb, vb, lr, beta1, beta2, weight_decay, eps, step);
        ctx.record(name + "1_adam-update", 0);
        ctx.register_timer(name + "adam-update", name + "0_adam-update", name + "1_adam-update");
    }

    auto get_b() { return b; }
    auto get_W() { return W; }
    auto get_G_W() { return G_W; }
    auto get_G_b() { return G_b; }
    // checkpoints (gcn::save / load): Adam's moments (after adam_state) and the step count
    auto get_mW() { return mW; }
    auto get_vW() { return vW; }
    auto get_mb() { return mb; }
    auto get_vb() { return vb; }
    bool has_adam_state() const { return has_moments; }
    std::size_t adam_steps() const { return has_moments ? step : 0; }
    void set_adam_steps(std::size_t s) { step = s; }
};

// Checkpoints, shared by gcn and dist_gcn (checkpoint.hpp has the file; INTEGRATION.md its layout).  A tensor of the
// model as the file sees it: the parameter and its two moments as one device matrix per replica (one on a single GPU).
template <typename r_t>
struct checkpoint_slot {
    std::string name;
    std::vector<dn_matrix<r_t>> p, m, v;      // m, v: empty handles while the model has not stepped
};

// the slots of one layer in file order: W, b, the residual linear's, the norm's
template <typename r_t, typename layer_t, typename pick_t>
void checkpoint_slots_of(layer_t &layer, std::size_t l, pick_t &&pick, std::vector<checkpoint_slot<r_t>> &out) {
    const auto s = std::to_string(l);
    const auto lins = layer.linears();
    for (std::size_t k = 0; k < lins.size(); k++) {
        const std::string pre = k ? "res_" : "";
        out.push_back({pre + "W" + s, pick(lins[k]->get_W()), pick(lins[k]->get_mW()), pick(lins[k]->get_vW())});
        out.push_back({pre + "b" + s, pick(lins[k]->get_b()), pick(lins[k]->get_mb()), pick(lins[k]->get_vb())});
    }
    if (auto *nm = layer.layer_norm_params()) {
        out.push_back({"gamma" + s, {nm->gamma}, {nm->mg}, {nm->vg}});
        out.push_back({"beta" + s, {nm->beta}, {nm->mb}, {nm->vb}});
    }
}

// host copy of the slots into a checkpoint whose configuration is already filled in; replica 0 is read.  `set(g)` makes
// replica g's device current.  The caller has synchronised.
template <typename r_t, typename set_t>
void checkpoint_download(mggcn::checkpoint &c, const std::vector<checkpoint_slot<r_t>> &slots, bool stepped, set_t &&set) {
    set(0);
    for (const auto &sl : slots) {
        mggcn::checkpoint_tensor t;
        t.name = sl.name, t.rows = (std::uint32_t)sl.p[0].n(), t.cols = (std::uint32_t)sl.p[0].m();
        t.data = sl.p[0].to_host();
        if (c.optimizer) {
            t.m = stepped ? sl.m[0].to_host() : std::vector<r_t>(t.size(), (r_t)0);
            t.v = stepped ? sl.v[0].to_host() : std::vector<r_t>(t.size(), (r_t)0);
        }
        c.tensors.push_back(std::move(t));
    }
}

// the file's tensors into every replica, in place (dn_matrix::init): the buffers keep their addresses, which the cached
// Adam tables hold.  A file without the optimiser section zeroes the moments.  The caller has synchronised and has run
// adam_state, so the moments exist.
template <typename r_t, typename set_t>
void checkpoint_upload(const mggcn::checkpoint &c, std::vector<checkpoint_slot<r_t>> &slots, set_t &&set) {
    mggcn_require(slots.size() == c.tensors.size(), "checkpoint: tensor count");
    for (std::size_t k = 0; k < slots.size(); k++) {
        const auto &t = c.tensors[k];
        auto &sl = slots[k];
        mggcn_require(t.name == sl.name && t.rows == sl.p[0].n() && t.cols == sl.p[0].m(), "checkpoint: tensor name or shape");
        for (std::size_t g = 0; g < sl.p.size(); g++) {
            set(g);
            sl.p[g].init(t.data);
            sl.m[g].init(c.optimizer ? t.m : std::vector<r_t>(t.size(), (r_t)0));
            sl.v[g].init(c.optimizer ? t.v : std::vector<r_t>(t.size(), (r_t)0));
        }
    }
}

template <typename r_t>
class linear : public linear_body<r_t, context, dn_matrix, dn_matrix> {
    using body = linear_body<r_t, context, dn_matrix, dn_matrix>;

public:
    linear(std::string name, std::size_t in, std::size_t out, bool backward_out = true, bool fused = false)
        : body(name, dn_matrix<r_t>(in, out), dn_matrix<r_t>(in, out), dn_matrix<r_t>(1, out), dn_matrix<r_t>(1, out), backward_out, fused) {
        this->W.init();
        this->b.init(std::sqrt((r_t)1.0 / 3));
    }

    void adam_tensors(std::vector<std::array<dn_matrix<r_t>, 4>> &out, std::vector<r_t> &wd, r_t weight_decay) const {
        out.push_back({this->W, this->G_W, this->mW, this->vW}); wd.push_back(weight_decay);    // W decays, b does not (reference :163)
        out.push_back({this->b, this->G_b, this->mb, this->vb}); wd.push_back((r_t)0);
    }
};

template <typename r_t>
class dist_row_linear : public linear_body<r_t, dist_context, dist_row_dn_matrix, repl_dn_matrix> {
    using body = linear_body<r_t, dist_context, dist_row_dn_matrix, repl_dn_matrix>;
    using rdn_t = repl_dn_matrix<r_t>;
    // G_W and G_b of a layer live in ONE buffer per GPU: [G_W | pad to 4 floats | G_b] -> a single in-place
    // all-reduce per layer (the reference all-reduces them separately, :236-240), run on the comm stream
    // while the backward pass goes on; awaited by finish_backward() / adam_update()
    rdn_t G_all;
    bool pending = false;

    static std::vector<mggcn::device_ptr<r_t>> alloc_flat(const dist_context &ctx, std::size_t len) {
        std::vector<mggcn::device_ptr<r_t>> t;
        for (std::size_t i = 0; i < ctx.size(); i++) {
            ctx[i].set();
            t.push_back(mggcn::device_malloc<r_t>(len));
            mggcn_memset_zero(t.back().get(), len * sizeof(r_t), ctx[i].stream(0));     // the padding takes part in the sum
        }
        return t;
    }
    static std::vector<mggcn::device_ptr<r_t>> views(const std::vector<mggcn::device_ptr<r_t>> &owner, std::size_t off) {
        std::vector<mggcn::device_ptr<r_t>> t;
        for (const auto &o : owner) t.push_back(mggcn::device_view(o, off));
        return t;
    }

    void reduce_gradients(const dist_context &ctx) override {
        const int cs = ctx.bcast_stream_id();
        ctx.record(this->name + "1_1_grad-local", 0);
        ctx.wait(this->name + "1_1_grad-local", cs);
        G_all.allreduce(ctx, cs);                                             // [G_W | G_b] summed over the GPUs
        ctx.record(this->name + "1_2_grad-reduced", cs);
        pending = true;
    }

public:
    dist_row_linear(const dist_context ctx, std::string name, std::size_t in, std::size_t out, bool backward_out = true, bool fused = false)
        : body(name, rdn_t(ctx, in, out), rdn_t(), rdn_t(ctx, 1, out), rdn_t(), backward_out, fused) {
        const std::size_t off_b = (in * out + 3) / 4 * 4;
        const auto G_flat = alloc_flat(ctx, off_b + out);
        this->G_W = rdn_t(ctx, in, out, G_flat);
        this->G_b = rdn_t(ctx, 1, out, views(G_flat, off_b));
        G_all = rdn_t(ctx, 1, off_b + out, G_flat);
        this->W.init(ctx);
        this->b.init(ctx, std::sqrt((r_t)1.0 / 3));
    }

    void finish_backward(const dist_context &ctx) override {
        if (pending) ctx.wait(this->name + "1_2_grad-reduced", 0);
        pending = false;
    }

    void adam_tensors(std::size_t gpu, std::vector<std::array<dn_matrix<r_t>, 4>> &out, std::vector<r_t> &wd, r_t weight_decay) const {
        out.push_back({this->W[gpu], this->G_W[gpu], this->mW[gpu], this->vW[gpu]}); wd.push_back(weight_decay);
        out.push_back({this->b[gpu], this->G_b[gpu], this->mb[gpu], this->vb[gpu]}); wd.push_back((r_t)0);
    }
};

// Layer normalisation of one layer (gcn::set_layer_norm; opt-in, single GPU only -- the reference has none): gamma (ones),
// beta (zeros), their gradients and Adam moments, and what the backward pass needs of the forward: xhat [n x out], rstd [n].
template <typename r_t>
struct layer_norm_state {
    dn_matrix<r_t> gamma, beta, G_gamma, G_beta, mg, vg, mb, vb, xhat, rstd;
    bool has_moments = false;
    std::size_t step = 0;

    layer_norm_state(std::size_t n, std::size_t out)
        : gamma(1, out), beta(1, out), G_gamma(1, out), G_beta(1, out), xhat(n, out), rstd(n, 1) {
        gamma.fill((r_t)1);
        beta.fill((r_t)0);
    }
    void adam_state(const context &ctx) {
        if (has_moments) return;
        mg = zeros_like(ctx, gamma); vg = zeros_like(ctx, gamma); mb = zeros_like(ctx, beta); vb = zeros_like(ctx, beta);
        has_moments = true;
        step = 0;
    }
    // rows of the model-wide Adam table: neither decays
    void adam_tensors(std::vector<std::array<dn_matrix<r_t>, 4>> &out, std::vector<r_t> &wd) const {
        out.push_back({gamma, G_gamma, mg, vg}); wd.push_back((r_t)0);
        out.push_back({beta, G_beta, mb, vb}); wd.push_back((r_t)0);
    }
    // the unfused chain linear::adam_update runs for b
    void adam_update(const context &ctx, r_t lr, r_t beta1, r_t beta2, r_t eps) {
        adam_state(ctx);
        step += 1;
        const r_t bc1 = 1 - std::pow(beta1, step), bc2 = 1 - std::pow(beta2, step);
        axpby(ctx, G_gamma, mg, 1 - beta1, beta1);
        axpby(ctx, G_beta, mb, 1 - beta1, beta1);
        aaxpby(ctx, G_gamma, vg, 1 - beta2, beta2);
        aaxpby(ctx, G_beta, vb, 1 - beta2, beta2);
        adam_final(ctx, gamma, mg, vg, lr, bc1, bc2, eps);
        adam_final(ctx, beta, mb, vb, lr, bc1, bc2, eps);
    }
};

// One GCN layer (reference :411-518 / :520-637), written once over the context, matrix, aggregation (sparse_linear /
// dist_sparse_linear) and linear types.  HW / G_HW alias the model-wide HW_buffer, AHW / G_out the layer's AHW_buffer
// (:433-434); the thin classes below allocate them.
template <typename r_t, typename ctx_t, typename dn_t, typename agg_t, typename linear_t>
class gcn_layer_body {
protected:
    std::string name;
    agg_t A;
    linear_t lin;
    std::optional<linear_t> res_lin;      // residual connection when in != out (reference :418, :430)
    bool residual_layer;
    dn_t HW, AHW, G_HW, G_out;            // HW_buffer / AHW_buffer / HW_buffer / AHW_buffer
    bool activation, backward_spmm, fused;
    dn_t H;
    // fused backward (set by the model): mask_input_grad -- my G_out GEMM applies leaky_relu'(H) of the layer
    // below; grad_premasked -- the G I receive already carries my own activation's mask
    bool mask_input_grad = false, grad_premasked = false;
    // dropout of my input (gcn::set_dropout; single GPU only): set by the model before every forward, empty = none.  In
    // place in the AHW buffer of the layer below: its backward reads that buffer for the SIGN of its activation only,
    // which scaling by 1 / (1 - p) > 0 keeps, and a dropped element gets a zero gradient from the call in backward().
    std::optional<dropout_call> drop;
    // layer normalisation between aggregation / linear and activation (gcn::set_layer_norm; single GPU only), with the
    // activation in the same launch on the fused path
    std::optional<layer_norm_state<r_t>> norm;

    void norm_forward(ctx_t ctx) {
        if constexpr (std::is_same_v<ctx_t, context>) {
            ctx.record(name + "0_0_norm", 0);
            layer_norm(ctx, AHW, AHW, norm->xhat, norm->rstd, norm->gamma, norm->beta, fused);
            ctx.record(name + "0_1_norm", 0);
            ctx.register_timer(name + "0_norm", name + "0_0_norm", name + "0_1_norm");
        } else {
            throw std::invalid_argument("layer norm is single-GPU only in the C++ layer");
        }
    }
    // G_in = AHW; act: apply leaky_relu'(act) to G first
    void norm_backward(ctx_t ctx, dn_t G, const dn_t *act) {
        if constexpr (std::is_same_v<ctx_t, context>) {
            ctx.record(name + "1_0_norm", 0);
            layer_norm_backward(ctx, G, act, norm->xhat, norm->rstd, norm->gamma, AHW, norm->G_gamma, norm->G_beta);
            ctx.record(name + "1_1_norm", 0);
            ctx.register_timer(name + "1_norm", name + "1_0_norm", name + "1_1_norm");
        } else {
            throw std::invalid_argument("layer norm is single-GPU only in the C++ layer");
        }
    }

    void apply_dropout(ctx_t ctx, dn_t M, const std::string &tag) {
        if constexpr (std::is_same_v<ctx_t, context>) {
            ctx.record(name + tag + "_0_dropout", 0);
            dropout(ctx, M, M, *drop);
            ctx.record(name + tag + "_1_dropout", 0);
            ctx.register_timer(name + tag + "_dropout", name + tag + "_0_dropout", name + tag + "_1_dropout");
        } else {
            throw std::invalid_argument("dropout is single-GPU only in the C++ layer");
        }
    }

    gcn_layer_body(std::string name, agg_t A, linear_t lin, std::optional<linear_t> res_lin, bool residual_layer, bool activation,
                   bool backward_spmm, bool fused)
        : name(name), A(A), lin(lin), res_lin(res_lin), residual_layer(residual_layer), activation(activation),
          backward_spmm(backward_spmm), fused(fused) {}

    // AHW = A (H W + 1 b^T) in the reference's order (:439-446); true when the SpMM's epilogue applied the activation
    virtual bool aggregate_linear(ctx_t ctx, dn_t H) {
        if (gemm_first()) {                      // out <= in: GEMM first
            lin(ctx, H, HW);
            if (fused && activation && !norm) { A(ctx, HW, AHW, true, MGGCN_SPMM_LEAKY_RELU); return true; }   // a norm carries the activation
            A(ctx, HW, AHW);
            return false;
        }
        A(ctx, H, HW);
        lin(ctx, HW, AHW);
        return false;
    }

    // the backward pass up to the gradient of my input (reference :460-489)
    dn_t input_gradient(ctx_t ctx, dn_t G) {
        auto T = G;
        if (norm && fused) {
            // one launch: leaky_relu'(AHW as the forward left it) unless G already carries it, then the norm's backward
            norm_backward(ctx, G, grad_premasked ? nullptr : &AHW);
            T = AHW;
        } else if (activation && !grad_premasked) {
            ctx.record(name + "1_0_activation", 0);
            leaky_relu_backward(ctx, AHW, G, AHW);
            ctx.record(name + "1_1_activation", 0);
            ctx.register_timer(name + "1_activation", name + "1_0_activation", name + "1_1_activation");
            T = AHW;
            if (norm) norm_backward(ctx, AHW, nullptr);
        }
        if (gemm_first()) {
            auto g = G_HW;
            if (backward_spmm) A.backward(ctx, T, g); else g = T;
            lin.backward(ctx, g, G_out, true, mask_input_grad ? &H : nullptr);
            return residual_backward(ctx, G, G_out);
        }
        lin.setX(H);
        lin.backward(ctx, T, G_HW);
        if (backward_spmm) { A.backward(ctx, G_HW, G_out); return residual_backward(ctx, G, G_out); }
        return residual_backward(ctx, G, G_HW);
    }

    // reference :484-487: the residual branch sees the incoming (unmasked) gradient and adds to G_out
    dn_t residual_backward(ctx_t ctx, dn_t G, dn_t out) {
        if (res_lin) res_lin->backward(ctx, G, out, false);
        else if (residual_layer) axpy(ctx, G, out, (r_t)1);
        return out;
    }

public:
    bool gemm_first() const { return HW.m() == AHW.m(); }           // out <= in (reference :439)
    bool has_activation() const { return activation; }
    bool has_residual() const { return residual_layer; }
    bool propagates() const { return lin.has_backward_out(); }
    void set_fused_backward(bool mask_input, bool premasked) { if (mask_input) mask_input_grad = true; if (premasked) grad_premasked = true; }
    void set_dropout_call(std::optional<dropout_call> d) { drop = d; }
    // on: a fresh norm (gamma = 1, beta = 0) if this layer has an activation; off: none
    void set_layer_norm(bool on) {
        if (on && activation) norm.emplace(AHW.n(), AHW.m());
        else norm.reset();
    }
    layer_norm_state<r_t> *layer_norm_params() { return norm ? &*norm : nullptr; }
    linear_t &linear_layer() { return lin; }
    std::vector<linear_t *> linears() {
        std::vector<linear_t *> v{&lin};
        if (res_lin) v.push_back(&*res_lin);
        return v;
    }

    auto operator()(ctx_t ctx, dn_t H) {
        if (drop) apply_dropout(ctx, H, "0");
        this->H = H;
        bool act_done = aggregate_linear(ctx, H);
        if (norm) { norm_forward(ctx); act_done = fused; }
        if (activation && !act_done) {
            ctx.record(name + "0_0_activation", 0);
            leaky_relu_forward(ctx, AHW, AHW);
            ctx.record(name + "0_1_activation", 0);
            ctx.register_timer(name + "0_activation", name + "0_0_activation", name + "0_1_activation");
        }
        if (res_lin) (*res_lin)(ctx, H, AHW, false);          // reference :453-456
        else if (residual_layer) axpy(ctx, H, AHW, (r_t)1);
        return AHW;
    }

    auto backward(ctx_t ctx, dn_t G) {
        auto out = input_gradient(ctx, G);
        if (drop) apply_dropout(ctx, out, "1");      // last: after the GEMM epilogue's leaky_relu' and the residual add
        return out;
    }

    void finish_backward(const ctx_t ctx) { for (auto *l : linears()) l->finish_backward(ctx); }
    void update(const ctx_t ctx, const r_t lr, const r_t wd) { for (auto *l : linears()) l->update(ctx, lr, wd); }
    void adam_update(const ctx_t ctx, const r_t lr, const r_t b1, const r_t b2, const r_t wd, const r_t eps) {
        for (auto *l : linears()) l->adam_update(ctx, lr, b1, b2, wd, eps);
        if constexpr (std::is_same_v<ctx_t, context>) { if (norm) norm->adam_update(ctx, lr, b1, b2, eps); }
    }
    auto b() { return lin.get_b(); }
    auto W() { return lin.get_W(); }
    auto GW() { return lin.get_G_W(); }
    auto Gb() { return lin.get_G_b(); }
};

template <typename x_t, typename v_t, typename r_t>
class gcn_layer : public gcn_layer_body<r_t, context, dn_matrix<r_t>, sparse_linear<x_t, v_t, r_t>, linear<r_t>> {
    using body = gcn_layer_body<r_t, context, dn_matrix<r_t>, sparse_linear<x_t, v_t, r_t>, linear<r_t>>;
    // optional, first layer only (gcn::set_hoist_first_aggregation): A_fwd . X computed once and kept
    bool hoist_input = false;
    dn_matrix<r_t> AX;
    const r_t *AX_src = nullptr;
    unsigned AX_generation = 0;

    bool aggregate_linear(context ctx, dn_matrix<r_t> H) override {
        if (!hoist_input) return body::aggregate_linear(ctx, H);
        // layer 0's aggregation is loop-invariant: A_fwd (X W + 1 b^T) = (A_fwd X) W + 1 b^T (A_fwd is row-stochastic,
        // X never changes between epochs): A_fwd X once, one SpMM fewer per epoch.  NOT the reference's epoch
        // (:437-446): an option, off by default.  The backward pass stays the reference's (G_W = X^T T, :954).
        auto &A = this->A;
        if (!AX.buffer() || AX_src != H.buffer() || AX.n() != this->AHW.n() || AX.m() != H.m() ||
            AX_generation != A.forward_matrix().generation()) {
            AX = dn_matrix<r_t>(this->AHW.n(), H.m());
            A(ctx, H, AX);
            AX_src = H.buffer();
            AX_generation = A.forward_matrix().generation();
        }
        this->lin(ctx, AX, this->AHW);
        this->lin.setX(H);
        return false;
    }

public:
    // A_fwd (1 b^T) = 1 b^T needs every row of A_fwd to sum to one: a vertex whose row of A_fwd is empty (no self-loop, nobody
    // points at it) would get 0 instead of b -- such a graph keeps the plain path.  (Re-)enabling drops the cached product:
    // the way to pick up an in-place change of the feature matrix, which the (buffer, shape, matrix generation) key cannot see.
    void set_hoist_input(bool on) {
        hoist_input = on && this->gemm_first() && !this->residual_layer && this->A.forward_matrix().every_row_nonempty();
        AX = dn_matrix<r_t>();
        AX_src = nullptr;
    }
    bool hoists_input() const { return hoist_input; }

    gcn_layer(std::string name, csr_matrix<x_t, v_t, r_t> A, csr_matrix<x_t, v_t, r_t> A_T, std::size_t in, std::size_t out,
              bool activation, bool residual_layer = false, bool backward_spmm = true,
              mggcn::device_ptr<r_t> HW_buffer = nullptr, bool fused = false, agg_dtype agg = agg_dtype::f32,
              mggcn::device_ptr<std::uint16_t> agg_buffer = nullptr, std::size_t agg_capacity = 0)
        : body(name, sparse_linear<x_t, v_t, r_t>(name, A, A_T, agg, agg_buffer, agg_capacity), linear<r_t>(name, in, out, backward_spmm, fused),
               in == out || !residual_layer ? std::nullopt : std::make_optional(linear<r_t>(name, in, out, backward_spmm, false)),
               residual_layer, activation, backward_spmm, fused) {
        const std::size_t mn = std::min(in, out);
        if (!HW_buffer) HW_buffer = mggcn::device_malloc<r_t>(std::max<std::size_t>(A.m(), A_T.n()) * mn);
        const auto AHW_buffer = mggcn::device_malloc<r_t>(std::max((std::size_t)A.n() * out, (std::size_t)A_T.n() * in));
        this->HW = dn_matrix<r_t>(A.m(), mn, HW_buffer);
        this->AHW = dn_matrix<r_t>(A.n(), out, AHW_buffer);
        this->G_HW = dn_matrix<r_t>(A_T.n(), mn, HW_buffer);
        this->G_out = dn_matrix<r_t>(A_T.n(), in, AHW_buffer);
    }
};

template <bool row_partition, typename x_t, typename v_t, typename r_t>
class dist_gcn_layer : public gcn_layer_body<r_t, dist_context, dist_row_dn_matrix<r_t>, dist_sparse_linear<row_partition, x_t, v_t, r_t>,
                                             dist_row_linear<r_t>> {
    using body = gcn_layer_body<r_t, dist_context, dist_row_dn_matrix<r_t>, dist_sparse_linear<row_partition, x_t, v_t, r_t>,
                                dist_row_linear<r_t>>;
    using csr_t = dist_row_csr_matrix<x_t, v_t, r_t>;
    using dn_t = dist_row_dn_matrix<r_t>;
    using bufs_t = std::vector<mggcn::device_ptr<r_t>>;

public:
    dist_gcn_layer(const dist_context ctx, std::string name, csr_t A, csr_t A_T, std::size_t in, std::size_t out, bool activation,
                   bool residual_layer = false, bool backward_spmm = true, bufs_t HW_buffer = {}, bufs_t bcast_buffer = {},
                   bufs_t bcast_buffer2 = {}, bool fused = false, dist_mode mode = dist_mode::allgather)
        : body(name, dist_sparse_linear<row_partition, x_t, v_t, r_t>(name, A, A_T, bcast_buffer, bcast_buffer2, mode),
               dist_row_linear<r_t>(ctx, name, in, out, backward_spmm, fused),
               in == out || !residual_layer ? std::nullopt : std::make_optional(dist_row_linear<r_t>(ctx, name, in, out, backward_spmm, false)),
               residual_layer, activation, backward_spmm, fused) {
        bufs_t AHW_buffer;                        // per GPU: its rows only
        for (std::size_t i = 0; i < ctx.size(); i++) {
            ctx[i].set();
            AHW_buffer.push_back(mggcn::device_malloc<r_t>(std::max(A.n() * out, A_T.n() * in) / ctx.size()));
        }
        this->HW = dn_t(ctx, A.m(), std::min(in, out), HW_buffer);
        this->AHW = dn_t(ctx, A.n(), out, AHW_buffer);
        this->G_HW = dn_t(ctx, A_T.n(), std::min(in, out), HW_buffer);
        this->G_out = dn_t(ctx, A_T.n(), in, AHW_buffer);
    }
};

// softmax: row max, exp(x - max), row sums by a GEMM with a ones vector, divide (reference :639-676)
template <typename r_t>
class softmax {
    dn_matrix<r_t> ones, H, H_R, maxs;
    const bool copy;

public:
    softmax(bool copy = true) : copy(copy) {}
    auto operator()(const context ctx, dn_matrix<r_t> temp) {
        if (copy) {
            if (!H.buffer()) H = dn_matrix<r_t>(temp.n(), temp.m());
            temp.copy_to(ctx, H);
        } else {
            H = temp;
        }
        if (!maxs.buffer()) maxs = dn_matrix<r_t>(H.n(), 1);
        max_rows(ctx, H, maxs);
        subtract_rows_exp(ctx, H, maxs, H);
        if (!ones.buffer()) { ones = dn_matrix<r_t>(H.m(), 1); ones.fill(1); }
        if (!H_R.buffer()) H_R = dn_matrix<r_t>(H.n(), 1);
        matmul(ctx, H, ones, H_R, (r_t)1, (r_t)0);
        scale_rows(ctx, H, H_R);
        return H;
    }
};

// Split-aware training (opt-in; the reference loads sets.bin and ignores it, src/main.cpp:85): S holds a set per row of
// the logits (0 train / 1 validation / 2 test, anything else in no split), the loss is taken over the n_train rows of
// train_set, every other row gets a zero gradient row, and a (loss sum, correct count) pair is kept per slot.
template <typename x_t>
struct loss_split {
    dn_matrix<x_t> S;            // this GPU's rows
    int train_set;
    std::size_t n_train;         // GLOBAL number of rows in train_set
};

inline std::size_t split_slot(std::int64_t s) { return s >= 0 && s <= 2 ? (std::size_t)s : 3; }

// rows per slot (train, val, test, other) of a host copy of the sets
template <typename x_t>
std::array<std::size_t, 4> split_counts(const std::vector<x_t> &sets) {
    std::array<std::size_t, 4> c{0, 0, 0, 0};
    for (const auto s : sets) c[split_slot((std::int64_t)s)]++;
    return c;
}

inline void check_train_set(int train_set) {
    if (train_set < 0 || train_set > 2) throw std::invalid_argument("train_set must be 0 (train), 1 (validation) or 2 (test)");
}
inline void check_somebody_trains(std::size_t n_train) {
    if (n_train == 0) throw std::invalid_argument("no vertex belongs to the training set: nothing to train on");
}

// (loss, acc) per slot from the eight sums and the four counts; a split without a row reports nan
template <typename r_t>
std::array<std::pair<r_t, r_t>, 4> split_metrics_of(const std::array<r_t, 8> &s, const std::array<std::size_t, 4> &counts) {
    std::array<std::pair<r_t, r_t>, 4> out;
    for (std::size_t k = 0; k < 4; k++)
        out[k] = counts[k] ? std::make_pair(s[2 * k] / (r_t)counts[k], s[2 * k + 1] / (r_t)counts[k])
                           : std::make_pair(std::numeric_limits<r_t>::quiet_NaN(), std::numeric_limits<r_t>::quiet_NaN());
    return out;
}

// The multi-label loss (opt-in, set_loss_bce; the reference has none): sixteen sums, (loss sum, TP, FP, FN) per slot, from
// mggcn_sigmoid_bce_from_f32.  micro-F1 = 2 TP / (2 TP + FP + FN), nan when nothing is positive and nothing predicted so.
template <typename r_t>
r_t micro_f1(r_t tp, r_t fp, r_t fn) {
    const r_t den = 2 * tp + fp + fn;
    return den != 0 ? 2 * tp / den : std::numeric_limits<r_t>::quiet_NaN();
}
// (loss, micro-F1) per slot: the loss is the mean over the slot's rows AND the m columns; a split without a row reports nan
template <typename r_t>
std::array<std::pair<r_t, r_t>, 4> bce_metrics_of(const std::array<r_t, 16> &s, const std::array<std::size_t, 4> &counts, std::size_t m) {
    std::array<std::pair<r_t, r_t>, 4> out;
    for (std::size_t k = 0; k < 4; k++)
        out[k] = counts[k] ? std::make_pair((r_t)(s[4 * k] / ((double)counts[k] * (double)m)), micro_f1(s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]))
                           : std::make_pair(std::numeric_limits<r_t>::quiet_NaN(), std::numeric_limits<r_t>::quiet_NaN());
    return out;
}

// One GPU's share of the loss: enqueues everything and leaves the sums in mapped pinned host memory -- {sum|log p_y|,
// #correct} over its rows, or one such pair per slot with a loss_split; the caller synchronises and reads
// (reference :785-818 / :890-930).
template <typename r_t, typename x_t>
class loss_kernels {
    softmax<r_t> softmax_layer;
    dn_matrix<r_t> G, L, T;
    dn_matrix<x_t> P;
    const bool copy, fused;
    mggcn::device_ptr<r_t> sums_;    // eight floats (sixteen allocated: the multi-label loss writes them all), written by the
                                     // kernels, read by the host after its sync
    bool bce_ = false;               // the multi-label loss instead of softmax cross-entropy (set_bce)
    std::size_t slots_ = 1;          // pairs the last call wrote: 1, or the 4 of a split-aware call
    bool planar_ = false;            // ... as all loss sums, then all correct counts (the unfused chain) instead of pair by pair

public:
    loss_kernels(bool copy, bool fused) : softmax_layer(copy), copy(copy), fused(fused) {}
    auto gradient() const { return G; }
    void set_bce(bool on) { bce_ = on; }
    bool bce() const { return bce_; }
    // the sixteen sums of the last multi-label call: (loss sum, TP, FP, FN) of train / val / test / other; without a
    // split every row is in the first slot
    std::array<r_t, 16> bce_sums() const {
        std::array<r_t, 16> out{};
        for (std::size_t k = 0; k < 16; k++) out[k] = sums_.get()[k];
        return out;
    }
    // the sums of the last call as (loss sum, correct count) pairs: the one pair of a plain call first and zeros behind
    // it, or train / val / test / other
    std::array<r_t, 8> sums() const {
        std::array<r_t, 8> out{};
        const r_t *s = sums_.get();
        for (std::size_t k = 0; k < slots_; k++) {
            out[2 * k] = planar_ ? s[k] : s[2 * k];
            out[2 * k + 1] = planar_ ? s[slots_ + k] : s[2 * k + 1];
        }
        return out;
    }

    // with a split: the gradient is scaled by 1 / n_train instead of 1 / n_global, rows outside train_set get a zero
    // gradient row, and a pair of sums is kept per slot
    void enqueue(context ctx, dn_matrix<r_t> H, dn_matrix<x_t> Y, std::size_t n_global,
                 std::optional<loss_split<x_t>> split = std::nullopt) {
        ctx.set();
        if (split) {
            check_train_set(split->train_set);
            check_somebody_trains(split->n_train);
        }
        if (!sums_) sums_ = mggcn::host_malloc<r_t>(16);
        slots_ = split ? 4 : 1;
        if (bce_) {                           // Y: the int32 [n x m] targets; one kernel, copy = true writes G elsewhere
            if (copy) {
                if (!G.buffer() || G.shape() != H.shape()) G = dn_matrix<r_t>(H.n(), H.m());
            } else {
                G = H;
            }
            const double rows = (double)(split ? split->n_train : n_global);
            mggcn_memset_zero(sums_.get(), 16 * sizeof(r_t), ctx.stream(0));
            sigmoid_bce(ctx, H, G, Y, split ? &split->S : nullptr, split ? split->train_set : 0,
                        (r_t)(1.0 / (rows * (double)H.m())), sums_.get());
            return;
        }
        const r_t scale = (r_t)1 / (r_t)(split ? split->n_train : n_global);
        if (fused && H.m() >= 1 && H.m() <= 1024) {     // the one-pass kernel's widths; any other runs the chain below
            if (copy) {                       // reference: copy, then in place (:653-656); here the pass writes elsewhere
                if (!G.buffer() || G.shape() != H.shape()) G = dn_matrix<r_t>(H.n(), H.m());
            } else {
                G = H;
            }
            mggcn_memset_zero(sums_.get(), 2 * slots_ * sizeof(r_t), ctx.stream(0));
            if (split) softmax_xent_split(ctx, H, G, Y, split->S, split->train_set, scale, sums_.get());
            else softmax_xent_fused(ctx, H, G, Y, scale, sums_.get());
            planar_ = false;
            return;
        }
        auto O = softmax_layer(ctx, H);
        if (!P.buffer()) P = dn_matrix<x_t>(Y.shape());
        max_row_indices(ctx, O, P);
        if (!L.buffer()) L = dn_matrix<r_t>(Y.shape());
        index_log_rows(ctx, O, Y, L);
        G = O;
        add_indexed_rows(ctx, G, Y, (r_t)-1);
        scale_mat(ctx, G, scale);
        if (split) select_rows_by_set(ctx, G, split->S, split->train_set);
        if (!T.buffer()) T = dn_matrix<r_t>(Y.shape());
        is_equal(ctx, Y, P, T);
        if (split) {
            abssum_by_set(ctx, L, split->S, sums_.get());
            abssum_by_set(ctx, T, split->S, sums_.get() + 4);
        } else {
            abssum(ctx, L, sums_.get());
            abssum(ctx, T, sums_.get() + 1);
        }
        planar_ = true;
    }
};

template <typename r_t, typename x_t>
class softmax_cross_entropy_loss {
    std::string name;
    loss_kernels<r_t, x_t> k;

public:
    softmax_cross_entropy_loss(std::string name, bool copy = true, bool fused = false) : name(name), k(copy, fused) {}

    // train on the rows with S == train_set (see loss_split); counted here, on the host.  clear_splits() turns it off.
    void set_splits(dn_matrix<x_t> S, int train_set = 0) {
        check_train_set(train_set);
        mggcn_require(S.m() == 1, "set_splits: the sets must be n x 1");
        const auto c = split_counts(S.to_host());
        check_somebody_trains(c[(std::size_t)train_set]);
        counts_ = c;
        split_ = loss_split<x_t>{S, train_set, c[(std::size_t)train_set]};
    }
    void clear_splits() { split_.reset(); }
    bool has_splits() const { return split_.has_value(); }
    // the eight sums ((loss sum, correct count) of train / val / test / other) and the four row counts of the last call
    auto split_sums() const { return k.sums(); }
    auto split_counts_global() const { return counts_; }
    auto split_metrics() const {
        return k.bce() ? bce_metrics_of<r_t>(k.bce_sums(), counts_, m_) : split_metrics_of<r_t>(k.sums(), counts_);
    }
    // Multi-label training (opt-in): Y becomes the int32 [n x m] target matrix (non-zero = positive), the loss sigmoid +
    // binary cross-entropy averaged over rows and columns, and every (loss, acc) pair this class returns a
    // (loss, micro-F1) pair; bce_sums() has the raw (loss sum, TP, FP, FN) per slot of the last call.
    void set_loss_bce(bool on = true) {
        if (on) mggcn_require(&mggcn_sigmoid_bce_from_f32 != nullptr, "this libmggcn_hip.so has no sigmoid-BCE loss (mggcn_sigmoid_bce_from_f32)");
        k.set_bce(on);
    }
    bool loss_bce() const { return k.bce(); }
    auto bce_sums() const { return k.bce_sums(); }

    auto operator()(context ctx, dn_matrix<r_t> H, dn_matrix<x_t> Y) {
        if (split_) mggcn_require(split_->S.n() == H.n(), "the sets and the logits differ in their row count");
        if (k.bce()) mggcn_require(Y.n() == H.n() && Y.m() == H.m(), "the multi-label targets must have the logits' shape");
        m_ = H.m();
        ctx.record(name + "0_loss-layer", 0);
        k.enqueue(ctx, H, Y, Y.n(), split_);
        ctx.record(name + "1_loss-layer", 0);
        ctx.register_timer(name + "loss-layer", name + "0_loss-layer", name + "1_loss-layer");
        ctx.sync();
        if (split_) return split_metrics()[(std::size_t)split_->train_set];         // the training split's pair
        if (k.bce()) return bce_metrics_of<r_t>(k.bce_sums(), {H.n(), 0, 0, 0}, H.m())[0];
        const auto s = k.sums();
        return std::make_pair(s[0] / H.n(), s[1] / H.n());
    }
    auto backward() { return k.gradient(); }

private:
    std::size_t m_ = 1;                                          // width of the last call's logits
    std::optional<loss_split<x_t>> split_;
    std::array<std::size_t, 4> counts_{0, 0, 0, 0};
};

template <typename r_t, typename x_t>
class dist_row_softmax_cross_entropy_loss {
    std::string name;
    std::vector<std::shared_ptr<loss_kernels<r_t, x_t>>> ks;    // one per GPU, shared with the commands in flight
    const bool copy, fused;
    dist_row_dn_matrix<r_t> G;

public:
    dist_row_softmax_cross_entropy_loss(std::string name, bool copy = true, bool fused = false) : name(name), copy(copy), fused(fused) {}

    // train on the rows with S == train_set: the global counts are summed here, on the host, over the P shards (as the
    // scalars are below); a GPU without a training row is fine
    void set_splits(dist_context ctx, dist_row_dn_matrix<x_t> Sd, int train_set = 0) {
        check_train_set(train_set);
        std::array<std::size_t, 4> c{0, 0, 0, 0};
        for (std::size_t i = 0; i < ctx.size(); i++) {
            const auto ci = split_counts(Sd[i].to_host());
            for (std::size_t k = 0; k < 4; k++) c[k] += ci[k];
        }
        check_somebody_trains(c[(std::size_t)train_set]);
        counts_ = c;
        Sd_ = Sd;
        train_set_ = train_set;
    }
    void clear_splits() { Sd_.reset(); }
    bool has_splits() const { return Sd_.has_value(); }
    auto split_sums() const { return sums_; }                   // global, of the last call
    auto split_counts_global() const { return counts_; }
    auto split_metrics() const { return split_metrics_of<r_t>(sums_, counts_); }

    auto operator()(dist_context ctx, dist_row_dn_matrix<r_t> H, dist_row_dn_matrix<x_t> Y) {
        if (copy) throw std::invalid_argument("dist loss with copy = true is not used by the reference CLI");
        while (ks.size() < ctx.size()) ks.push_back(std::make_shared<loss_kernels<r_t, x_t>>(copy, fused));
        ctx.record(name + "0_loss-layer", 0);
        for (std::size_t i = 0; i < ctx.size(); i++) {           // global n (reference :908); S's handle is captured by value,
            std::optional<loss_split<x_t>> sp;                   // like the other matrices
            if (Sd_) sp = loss_split<x_t>{(*Sd_)[i], train_set_, counts_[(std::size_t)train_set_]};
            ctx.on(i, [k = ks[i], c = ctx[i], h = H[i], y = Y[i], n = Y.n(), sp] { k->enqueue(c, h, y, n, sp); });
        }
        ctx.record(name + "1_loss-layer", 0);
        ctx.register_timer(name + "loss-layer", name + "0_loss-layer", name + "1_loss-layer");
        ctx.sync();
        sums_.fill(0);
        for (std::size_t i = 0; i < ctx.size(); i++) {          // host sum of the per-GPU sums, in GPU order (reference :929)
            const auto s = ks[i]->sums();
            for (std::size_t k = 0; k < 8; k++) sums_[k] += s[k];
        }
        G = H;                                                   // copy = false: gradient in place, as in dist_gcn
        return Sd_ ? split_metrics()[(std::size_t)train_set_] : std::make_pair(sums_[0] / H.n(), sums_[1] / H.n());
    }
    auto backward() { return G; }

private:
    int train_set_ = 0;
    std::optional<dist_row_dn_matrix<x_t>> Sd_;                  // set: the splits are on
    std::array<std::size_t, 4> counts_{0, 0, 0, 0};
    std::array<r_t, 8> sums_{};                                  // (loss sum, correct count) pairs of the last call, see loss_kernels
};

// fused backward: layer i+1's G_out GEMM applies layer i's leaky_relu' -- possible when layer i+1 is GEMM-first
// (its G_out comes out of a GEMM, reference :479-481) and propagates a gradient at all
template <typename layers_t>
void link_fused_backward(layers_t &layers, bool fused) {
    for (std::size_t i = 0; i + 1 < layers.size(); i++) {
        // (a residual branch needs the UNMASKED incoming gradient and adds to G_out afterwards: no fusion there)
        const bool ok = fused && layers[i].has_activation() && layers[i + 1].gemm_first() && layers[i + 1].propagates() &&
                        !layers[i].has_residual() && !layers[i + 1].has_residual();
        layers[i + 1].set_fused_backward(ok, false);
        layers[i].set_fused_backward(false, ok);
    }
}

template <typename x_t, typename v_t, typename r_t>
class gcn {
    std::vector<gcn_layer<x_t, v_t, r_t>> layers_;
    softmax_cross_entropy_loss<r_t, std::int32_t> loss_layer;
    mggcn::device_ptr<r_t> HW_buffer;
    agg_dtype agg_ = agg_dtype::f32;
    mggcn::device_ptr<std::uint16_t> agg_buffer_;

public:
    // normalises A by column, A_T = A^T, layers get (A_T, A) (reference :946-955)
    // agg: storage of the SpMMs' gathered operand (agg_dtype::bf16: one bf16 scratch of n x the widest SpMM width)
    gcn(csr_matrix<x_t, v_t, r_t> A, std::vector<std::size_t> sizes, bool residual_layer = false, bool fused = true,
        agg_dtype agg = agg_dtype::f32)
        : loss_layer(std::to_string(sizes.size() - 1) + "_", residual_layer, fused), agg_(agg) {
        for (auto s : sizes) sizes_.push_back((std::uint32_t)s);
        residual_ = residual_layer;
        A.normalize(true);
        auto A_T = A.transpose();
        std::size_t max_d = 0;
        for (std::size_t i = 0; i + 1 < sizes.size(); i++) max_d = std::max(max_d, std::min(sizes[i], sizes[i + 1]));
        HW_buffer = mggcn::device_malloc<r_t>(std::max<std::size_t>(A.n(), A.m()) * max_d);
        const std::size_t agg_capacity = agg == agg_dtype::bf16 ? std::max<std::size_t>(A.n(), A.m()) * max_d : 0;
        if (agg_capacity) agg_buffer_ = mggcn::device_malloc<std::uint16_t>(agg_capacity);
        for (std::size_t i = 1; i < sizes.size(); i++)
            layers_.emplace_back(std::to_string(i - 1) + "_", A_T, A, sizes[i - 1], sizes[i], i + 1 < sizes.size(), residual_layer,
                                 i != 1, HW_buffer, fused, agg, agg_buffer_, agg_capacity);
        link_fused_backward(layers_, fused);
        fused_ = fused;
        // the SpMM plans of the model, built side by side now instead of one by one inside the first epoch
        std::vector<typename csr_matrix<x_t, v_t, r_t>::plan_want> wants;
        const int dev = mggcn_get_device();
        for (std::size_t i = 1; i < sizes.size(); i++) {
            wants.push_back({A_T, std::min(sizes[i - 1], sizes[i]), dev});             // forward multiplies by A_T (:954)
            if (i != 1) wants.push_back({A, std::min(sizes[i - 1], sizes[i]), dev});   // the first layer's backward SpMM is skipped
        }
        csr_matrix<x_t, v_t, r_t>::prebuild_plans(wants);
    }

    // Optional mode (never the reference's epoch): pre-compute the first layer's aggregation A_fwd . X once -- valid while
    // the SAME feature matrix is passed every epoch (full-graph training does); 6 instead of 7 SpMMs per epoch on the
    // Reddit model.  `mg_gcn` turns it on with MGGCN_HOIST_FIRST_AGGREGATION=1.
    // (fp32 aggregation only: with bf16 the hoisted product would round X instead of X W)
    void set_hoist_first_aggregation(bool on) {
        mggcn_require(!on || agg_ == agg_dtype::f32, "hoist_first_aggregation needs the f32 aggregation");
        layers_.front().set_hoist_input(on);
    }

    // test constructor with given weights (reference :957-963)
    gcn(csr_matrix<x_t, v_t, r_t> A, std::vector<std::size_t> sizes, std::vector<std::pair<std::vector<r_t>, std::vector<r_t>>> weights)
        : gcn(A, sizes) {
        for (std::size_t i = 0; i < layers_.size(); i++) {
            layers_[i].W().init(weights[i].first);
            layers_[i].b().init(weights[i].second);
        }
    }

    // the plain forward never drops; train_forward is the training forward
    auto operator()(const context ctx, dn_matrix<r_t> H) {
        arm_dropout(false);
        return forward(ctx, H);
    }
    auto train_forward(const context ctx, dn_matrix<r_t> H, dn_matrix<std::int32_t> Y) {
        arm_dropout(true);
        H = forward(ctx, H);
        return loss_layer(ctx, H, Y);
    }
    // Dropout (opt-in; the reference has none): train_forward drops the input of every layer but the first -- the
    // activated output of the layer below, in place; the features are the caller's buffer and are not dropped -- with the
    // mask of mggcn_dropout_f32 for (seed, stream = epoch * 64 + layer), never stored: backward() regenerates it.  epoch
    // counts the train_forward calls since set_dropout.  p = 0 switches it off (nothing is launched);
    // std::invalid_argument for a p outside [0, 1) or more than 64 layers, before any device work.
    // epoch: the number the next training forward gets (a loaded checkpoint continues its run's count)
    void set_dropout(double p, std::uint64_t seed = 0, std::size_t epoch = 0) {
        const auto d = dropout_params(p, seed);
        mggcn_require(p == 0.0 || layers_.size() <= 64, "dropout supports at most 64 layers");
        dropout_ = p > 0.0 ? std::make_optional(d) : std::nullopt;
        dropout_p_ = p, dropout_seed_ = seed;
        dropout_epoch_ = epoch;
    }
    std::size_t dropout_epoch() const { return dropout_epoch_; }
    // Layer normalisation (opt-in; the reference has none): every layer but the last normalises its rows between
    // aggregation / linear and activation (mggcn_layer_norm_forward_f32), the activation in the same launch on the fused
    // path; gamma (ones) and beta (zeros) are trained by Adam without weight decay.  It has no training mode: the plain
    // forward runs the same kernels.  Switching it on (again) starts from fresh parameters; off launches nothing new.
    void set_layer_norm(bool on) {
        if (on) require_layer_norm();
        for (auto &l : layers_) l.set_layer_norm(on);
        adam_ = adam_table<r_t>();               // the table holds raw pointers: rebuilt with the next step
    }
    // Train on one split (opt-in; the reference loads sets.bin and ignores it, src/main.cpp:85): S[i] is vertex i's set
    // (0 train / 1 validation / 2 test, anything else in no split).  From here on train_forward returns the loss and
    // accuracy of train_set; split_metrics() has every split's pair of the last epoch (train, val, test, other) from the
    // same pass.  std::invalid_argument for a bad train_set or when no vertex trains, before any device work.
    void set_splits(dn_matrix<std::int32_t> S, int train_set = 0) { loss_layer.set_splits(S, train_set); }
    void clear_splits() { loss_layer.clear_splits(); }
    auto split_metrics() const { return loss_layer.split_metrics(); }
    auto split_counts() const { return loss_layer.split_counts_global(); }
    // Multi-label training (opt-in; the reference has none): see softmax_cross_entropy_loss::set_loss_bce.  Y of
    // train_forward is then the int32 [n x sizes.back()] target matrix and the pairs are (loss, micro-F1).
    void set_loss_bce(bool on = true) { loss_layer.set_loss_bce(on); }
    auto bce_sums() const { return loss_layer.bce_sums(); }
    void backward(const context ctx) {
        auto G = loss_layer.backward();
        for (auto l = layers_.rbegin(); l != layers_.rend(); l++) G = l->backward(ctx, G);
    }
    void update(const context ctx, const r_t lr, const r_t wd) { for (auto &l : layers_) l.update(ctx, lr, wd); }
    void adam_update(const context ctx, const r_t lr, const r_t b1, const r_t b2, const r_t wd, const r_t eps) {
        if (!fused_) { for (auto &l : layers_) l.adam_update(ctx, lr, b1, b2, wd, eps); return; }
        // ONE launch for every parameter tensor of the model (reference: 7 launches per layer, :146-172, :990-994)
        std::size_t step = 0;
        for (auto &l : layers_)
            for (auto *lin : l.linears()) { lin->adam_state(ctx); step = lin->bump_step(); }
        for (auto &l : layers_)
            if (auto *nm = l.layer_norm_params()) { nm->adam_state(ctx); nm->step = step; }
        if (!adam_ || adam_wd_ != wd) {
            std::vector<std::array<dn_matrix<r_t>, 4>> t;
            std::vector<r_t> w;
            for (auto &l : layers_) {
                for (auto *lin : l.linears()) lin->adam_tensors(t, w, wd);
                if (auto *nm = l.layer_norm_params()) nm->adam_tensors(t, w);
            }
            adam_ = adam_table<r_t>(ctx, t, w);
            adam_wd_ = wd;
        }
        ctx.record("0_adam-update", 0);
        adam_.step(ctx, lr, b1, b2, (r_t)(1 - std::pow(b1, step)), (r_t)(1 - std::pow(b2, step)), eps);
        ctx.record("1_adam-update", 0);
        ctx.register_timer("adam-update", "0_adam-update", "1_adam-update");
    }
    auto &layers() { return layers_; }

    // Checkpoints (opt-in; the reference writes nothing): the file of checkpoint.hpp -- configuration, every parameter,
    // Adam's moments and step count (optimizer), the dropout state (p, seed, next epoch).  Execution options (fused, the
    // aggregation dtype, hoisting) are not stored.  state() is the host copy that save() writes.
    mggcn::checkpoint state(const context ctx, bool optimizer = true) {
        ctx.sync();
        auto c = describe();
        c.optimizer = optimizer;
        c.step = optimizer ? adam_steps() : 0;
        checkpoint_download(c, slots(), layers_.front().linear_layer().has_adam_state(), [&](std::size_t) { ctx.set(); });
        return c;
    }
    void save(const context ctx, const std::string &path, bool optimizer = true) { state(ctx, optimizer).write(path); }
    // Compares the file's configuration with the model's first: mggcn::checkpoint_error naming the first difference
    // ("sizes: file [..], model [..]"; the layer type first: an attention model's file is "model: file gat, model gcn",
    // checkpoint::mismatch) before a single device write.  Then parameters and moments are written in place,
    // every step count is restored (a file without the optimiser section resets Adam: zero moments, step 0) and
    // set_dropout gets the file's (p, seed, epoch).
    void load(const context ctx, const std::string &path) { load_state(ctx, mggcn::checkpoint::read(path), path); }
    void load_state(const context ctx, const mggcn::checkpoint &c, const std::string &path = "checkpoint") {
        const auto mine = describe();
        const auto bad = c.mismatch(mine.sizes, mine.residual_layer, mine.norm, mine.loss);
        if (!bad.empty()) throw mggcn::checkpoint_error(path + ": " + bad);
        set_dropout(c.dropout_p, c.dropout_seed, (std::size_t)c.dropout_epoch);
        for (auto &l : layers_) {
            for (auto *lin : l.linears()) lin->adam_state(ctx);
            if (auto *nm = l.layer_norm_params()) nm->adam_state(ctx);
        }
        ctx.sync();
        auto sl = slots();
        checkpoint_upload(c, sl, [&](std::size_t) { ctx.set(); });
        for (auto &l : layers_) {
            for (auto *lin : l.linears()) lin->set_adam_steps((std::size_t)c.step);
            if (auto *nm = l.layer_norm_params()) nm->step = (std::size_t)c.step;
        }
        ctx.sync();
    }
    // Adam steps taken so far (a loaded checkpoint's count included)
    std::size_t adam_steps() { return layers_.front().linear_layer().adam_steps(); }

private:
    mggcn::checkpoint describe() {
        mggcn::checkpoint c;
        c.sizes = sizes_, c.residual_layer = residual_;
        for (auto &l : layers_) if (l.layer_norm_params()) c.norm = 1;
        c.loss = loss_layer.loss_bce() ? 1 : 0;
        c.dropout_p = dropout_ ? dropout_p_ : 0.0, c.dropout_seed = dropout_seed_, c.dropout_epoch = dropout_epoch_;
        return c;
    }
    std::vector<checkpoint_slot<r_t>> slots() {
        std::vector<checkpoint_slot<r_t>> out;
        auto one = [](dn_matrix<r_t> t) { return std::vector<dn_matrix<r_t>>{t}; };
        for (std::size_t l = 0; l < layers_.size(); l++) checkpoint_slots_of<r_t>(layers_[l], l, one, out);
        return out;
    }
    std::vector<std::uint32_t> sizes_;
    bool residual_ = false;
    double dropout_p_ = 0;
    std::uint64_t dropout_seed_ = 0;

    auto forward(const context ctx, dn_matrix<r_t> H) {
        for (auto &layer : layers_) H = layer(ctx, H);
        return H;
    }
    // hands every layer but the first its call of this forward; a training forward takes the epoch number and moves it on
    void arm_dropout(bool training) {
        const bool on = training && dropout_;
        for (std::size_t l = 0; l < layers_.size(); l++) {
            std::optional<dropout_call> d;
            if (on && l > 0) { d = dropout_; d->stream = (std::uint32_t)(dropout_epoch_ * 64 + l); }
            layers_[l].set_dropout_call(d);
        }
        if (on) dropout_epoch_++;
    }

    bool fused_ = true;
    adam_table<r_t> adam_;
    r_t adam_wd_ = 0;
    std::optional<dropout_call> dropout_;
    std::size_t dropout_epoch_ = 0;
};

template <bool row_partition, typename x_t, typename v_t, typename r_t>
class dist_gcn {
    using csr_t = dist_row_csr_matrix<x_t, v_t, r_t>;
    using dn_t = dist_row_dn_matrix<r_t>;
    using idn_t = dist_row_dn_matrix<std::int32_t>;
    using bufs_t = std::vector<mggcn::device_ptr<r_t>>;
    std::vector<dist_gcn_layer<row_partition, x_t, v_t, r_t>> layers_;
    dist_row_softmax_cross_entropy_loss<r_t, std::int32_t> loss_layer;
    bufs_t HW_buffer, bcast_buffer, bcast_buffer2;

public:
    // per-GPU HW_buffer + receive buffers shared by all layers (reference :1016-1021).  The
    // all-gather schedule keeps the whole gathered B resident per GPU (n x max_d floats).
    dist_gcn(const dist_context ctx, csr_t A, csr_t A_T, std::vector<std::size_t> sizes, bool residual_layer = false,
             bool fused = true, dist_mode mode = dist_mode::allgather)
        : loss_layer(std::to_string(sizes.size() - 1) + "_", residual_layer, fused) {
        for (auto s : sizes) sizes_.push_back((std::uint32_t)s);
        residual_ = residual_layer;
        std::size_t max_d = 0;
        for (std::size_t i = 0; i + 1 < sizes.size(); i++) max_d = std::max(max_d, std::min(sizes[i], sizes[i + 1]));
        const std::size_t nmax = std::max(A.n(), A.m()), shard = nmax * max_d / ctx.size();
        for (std::size_t i = 0; i < ctx.size(); i++) {
            ctx[i].set();
            HW_buffer.push_back(mggcn::device_malloc<r_t>(shard));
            bcast_buffer.push_back(mggcn::device_malloc<r_t>(mode == dist_mode::rounds ? shard : nmax * max_d));
            bcast_buffer2.push_back(mggcn::device_malloc<r_t>(shard));
        }
        for (std::size_t i = 1; i < sizes.size(); i++)
            layers_.emplace_back(ctx, std::to_string(i - 1) + "_", A_T, A, sizes[i - 1], sizes[i], i + 1 < sizes.size(), residual_layer,
                                 i != 1, HW_buffer, bcast_buffer, bcast_buffer2, fused, mode);
        link_fused_backward(layers_, fused);
        fused_ = fused;
    }

    auto operator()(const dist_context ctx, dn_t H) {
        for (auto &layer : layers_) H = layer(ctx, H);
        return H;
    }
    auto train_forward(const dist_context ctx, dn_t H, idn_t Y) {
        H = operator()(ctx, H);
        return loss_layer(ctx, H, Y);
    }
    // see gcn::set_splits; Sd: the sets, sharded like the labels
    void set_splits(const dist_context ctx, idn_t Sd, int train_set = 0) { loss_layer.set_splits(ctx, Sd, train_set); }
    void clear_splits() { loss_layer.clear_splits(); }
    auto split_metrics() const { return loss_layer.split_metrics(); }
    auto split_counts() const { return loss_layer.split_counts_global(); }
    void backward(const dist_context ctx) {
        auto G = loss_layer.backward();
        for (auto l = layers_.rbegin(); l != layers_.rend(); l++) G = l->backward(ctx, G);
        for (auto &l : layers_) l.finish_backward(ctx);           // gradients are summed over the GPUs from here on
    }
    void adam_update(const dist_context ctx, const r_t lr, const r_t b1, const r_t b2, const r_t wd, const r_t eps) {
        if (!fused_) { for (auto &l : layers_) l.adam_update(ctx, lr, b1, b2, wd, eps); return; }
        std::size_t step = 0;
        for (auto &l : layers_) {
            l.finish_backward(ctx);
            for (auto *lin : l.linears()) { lin->adam_state(ctx); step = lin->bump_step(); }
        }
        if (adam_.size() != ctx.size() || adam_wd_ != wd) {
            adam_.clear();
            for (std::size_t g = 0; g < ctx.size(); g++) {
                std::vector<std::array<dn_matrix<r_t>, 4>> t;
                std::vector<r_t> w;
                for (auto &l : layers_)
                    for (auto *lin : l.linears()) lin->adam_tensors(g, t, w, wd);
                adam_.push_back(std::make_shared<adam_table<r_t>>(ctx[g], t, w));
            }
            adam_wd_ = wd;
        }
        ctx.record("0_adam-update", 0);
        for (std::size_t g = 0; g < ctx.size(); g++)
            ctx.on(g, [t = adam_[g], c = ctx[g], lr, b1, b2, c1 = (r_t)(1 - std::pow(b1, step)), c2 = (r_t)(1 - std::pow(b2, step)), eps] {
                t->step(c, lr, b1, b2, c1, c2, eps);
            });
        ctx.record("1_adam-update", 0);
        ctx.register_timer("adam-update", "0_adam-update", "1_adam-update");
    }
    auto &layers() { return layers_; }

    // Checkpoints: see gcn::save / load -- the same file, so a checkpoint of the single-GPU model loads here at any P and
    // the other way round.  GPU 0's replica is written (the replicas are bitwise equal); a load initialises every
    // replica.  These classes have no layer norm, multi-label loss or dropout: a file that has one is refused.
    mggcn::checkpoint state(const dist_context ctx, bool optimizer = true) {
        ctx.sync();
        auto c = describe();
        c.optimizer = optimizer;
        c.step = optimizer ? adam_steps() : 0;
        checkpoint_download(c, slots(ctx), layers_.front().linear_layer().has_adam_state(), [&](std::size_t g) { ctx[g].set(); });
        return c;
    }
    void save(const dist_context ctx, const std::string &path, bool optimizer = true) { state(ctx, optimizer).write(path); }
    void load(const dist_context ctx, const std::string &path) { load_state(ctx, mggcn::checkpoint::read(path), path); }
    void load_state(const dist_context ctx, const mggcn::checkpoint &c, const std::string &path = "checkpoint") {
        const auto mine = describe();
        const auto bad = c.mismatch(mine.sizes, mine.residual_layer, mine.norm, mine.loss);
        if (!bad.empty()) throw mggcn::checkpoint_error(path + ": " + bad);
        if (c.dropout_p > 0.0) throw mggcn::checkpoint_error(path + ": dropout: file " + std::to_string(c.dropout_p) + ", and dropout is single-GPU only in the C++ layer");
        for (auto &l : layers_)
            for (auto *lin : l.linears()) lin->adam_state(ctx);
        ctx.sync();
        auto sl = slots(ctx);
        checkpoint_upload(c, sl, [&](std::size_t g) { ctx[g].set(); });
        for (auto &l : layers_)
            for (auto *lin : l.linears()) lin->set_adam_steps((std::size_t)c.step);
        ctx.sync();
    }
    std::size_t adam_steps() { return layers_.front().linear_layer().adam_steps(); }

private:
    mggcn::checkpoint describe() const {
        mggcn::checkpoint c;
        c.sizes = sizes_, c.residual_layer = residual_;
        return c;
    }
    std::vector<checkpoint_slot<r_t>> slots(const dist_context &ctx) {
        std::vector<checkpoint_slot<r_t>> out;
        auto all = [&ctx](repl_dn_matrix<r_t> t) {
            std::vector<dn_matrix<r_t>> v;
            for (std::size_t g = 0; g < ctx.size() && g < t.size(); g++) v.push_back(t[g]);
            return v;
        };
        for (std::size_t l = 0; l < layers_.size(); l++) checkpoint_slots_of<r_t>(layers_[l], l, all, out);
        return out;
    }
    std::vector<std::uint32_t> sizes_;
    bool residual_ = false;
    bool fused_ = true;
    std::vector<std::shared_ptr<adam_table<r_t>>> adam_;     // one per GPU, shared with the commands in flight
    r_t adam_wd_ = 0;
};
