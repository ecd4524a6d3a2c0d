// checkpoint.hpp -- the checkpoint file, host only: nothing from HIP is included, plain g++ compiles it.
//
// The layout is documented byte by byte in INTEGRATION.md ("Checkpoint file"); datasets.py (write_checkpoint /
// read_checkpoint) is the numpy twin and both produce the same bytes for the same state:
//
//   "MGGCNCKP" | u32 version = 1 | u32 L | u32 sizes[L] | u32 residual_layer | u32 norm (0 none, 1 layer) |
//   u32 loss (0 softmax, 1 bce) | u32 optimizer (0 / 1) | f64 dropout p | u64 dropout seed | u64 dropout epoch |
//   u64 Adam step | u32 T | T x { u32 name length | name | u32 rows | u32 cols | f32 payload[rows * cols] } |
//   optimizer = 1: T x { f32 m[rows * cols] | f32 v[rows * cols] } in the order of the tensors | end of file
//
// An attention model (Python's gat and dist_gat; this layer has none and only refuses such a file by name) writes version 3:
// the same file with one block between `loss` and `optimizer`,
//
//   u32 model (1 gat) | u32 variant (1 v1, 2 v2) | u32 heads[L - 1] | f64 attn_slope | f64 attention dropout p
//
// residual_layer = norm = 0, and per layer W<l>, b<l>, att<l>.  Version 2 was never written; it is refused.
//
// All integers and floats little-endian (the hosts this runs on are).  The reader checks every length against the file's
// size before it allocates or copies; a truncated file, trailing bytes, a wrong magic or an unknown version is a
// checkpoint_error that names the file.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace mggcn {

class checkpoint_error : public std::runtime_error {
public:
    explicit checkpoint_error(const std::string &what) : std::runtime_error(what) {}
};

struct checkpoint_tensor {
    std::string name;
    std::uint32_t rows = 0, cols = 0;
    std::vector<float> data, m, v;       // m, v: Adam's moments, filled when the file has the optimiser section
    std::size_t size() const { return (std::size_t)rows * cols; }
};

struct checkpoint {
    static constexpr const char *magic = "MGGCNCKP";
    static constexpr std::uint32_t version = 1;              // model == 0 (gcn)
    static constexpr std::uint32_t version_attention = 3;    // model == 1 (gat)
    static constexpr std::uint32_t max_sizes = 4096;
    static constexpr std::uint32_t max_heads = 16, max_attention_width = 1024;      // the limits of the GAT kernels

    std::vector<std::uint32_t> sizes;
    bool residual_layer = false;
    std::uint32_t norm = 0;              // 0 none, 1 layer
    std::uint32_t loss = 0;              // 0 softmax, 1 bce
    bool optimizer = false;
    double dropout_p = 0;
    std::uint64_t dropout_seed = 0, dropout_epoch = 0, step = 0;
    // version 3 only: model 0 is a gcn file (version 1), which has none of these
    std::uint32_t model = 0;             // 0 gcn, 1 gat
    std::uint32_t variant = 0;           // 1 v1, 2 v2
    std::vector<std::uint32_t> heads;    // one per layer
    double attn_slope = 0, attn_dropout_p = 0;
    std::vector<checkpoint_tensor> tensors;

    static const char *norm_name(std::uint32_t n) { return n == 1 ? "layer" : "none"; }
    static const char *loss_name(std::uint32_t l) { return l == 1 ? "bce" : "softmax"; }
    static const char *model_name(std::uint32_t m) { return m == 1 ? "gat" : "gcn"; }

    // (name, rows, cols) of every parameter tensor the configuration implies, in file order
    // (model 1: W<l>, b<l>, att<l> -- [in x out], [1 x out], [2 x out] for variant 1, [in x 2 out], [1 x 2 out], [1 x out] for 2;
    // the caller has checked out <= max_attention_width)
    static std::vector<checkpoint_tensor> expected(const std::vector<std::uint32_t> &sizes, bool residual_layer, std::uint32_t norm,
                                                   std::uint32_t model = 0, std::uint32_t variant = 0) {
        std::vector<checkpoint_tensor> out;
        auto add = [&out](const std::string &name, std::uint32_t r, std::uint32_t c) {
            checkpoint_tensor t;
            t.name = name, t.rows = r, t.cols = c;
            out.push_back(std::move(t));
        };
        for (std::size_t l = 0; l + 1 < sizes.size(); l++) {
            const auto i = sizes[l], o = sizes[l + 1];
            const auto s = std::to_string(l);
            if (model == 1) {
                const auto z = variant == 2 ? 2 * o : o;
                add("W" + s, i, z), add("b" + s, 1, z), add("att" + s, variant == 2 ? 1 : 2, o);
                continue;
            }
            add("W" + s, i, o), add("b" + s, 1, o);
            if (residual_layer && i != o) add("res_W" + s, i, o), add("res_b" + s, 1, o);
            if (norm == 1 && l + 2 < sizes.size()) add("gamma" + s, 1, o), add("beta" + s, 1, o);
        }
        return out;
    }

    const checkpoint_tensor *find(const std::string &name) const {
        for (const auto &t : tensors)
            if (t.name == name) return &t;
        return nullptr;
    }

    // "" when the configurations agree, else the first difference as "<field>: file <x>, model <y>"
    static std::string list(const std::vector<std::uint32_t> &v) {
        std::string s = "[";
        for (std::size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
        return s + "]";
    }
    std::string mismatch(const std::vector<std::uint32_t> &m_sizes, bool m_residual, std::uint32_t m_norm, std::uint32_t m_loss,
                         std::uint32_t m_model = 0) const {
        if (model != m_model) return std::string("model: file ") + model_name(model) + ", model " + model_name(m_model);
        if (sizes != m_sizes) return "sizes: file " + list(sizes) + ", model " + list(m_sizes);
        if (residual_layer != m_residual)
            return std::string("residual_layer: file ") + (residual_layer ? "true" : "false") + ", model " + (m_residual ? "true" : "false");
        if (norm != m_norm) return std::string("norm: file ") + norm_name(norm) + ", model " + norm_name(m_norm);
        if (loss != m_loss) return std::string("loss: file ") + loss_name(loss) + ", model " + loss_name(m_loss);
        return "";
    }

    // what is wrong with the attention block next to the header, or ""; the writer and the reader share it
    std::string attention_problem() const {
        if (residual_layer || norm) return "unknown option value (residual_layer or norm in an attention model's file)";
        if (variant != 1 && variant != 2) return "unknown variant value " + std::to_string(variant);
        if (heads.size() + 1 != sizes.size()) return std::to_string(heads.size()) + " heads for " + std::to_string(sizes.size() - 1) + " layers";
        for (std::size_t l = 0; l < heads.size(); l++) {
            const auto h = heads[l], o = sizes[l + 1];
            const auto layer = "layer " + std::to_string(l);
            if (h < 1 || h > max_heads) return layer + " has " + std::to_string(h) + " heads, not 1.." + std::to_string(max_heads);
            if (o > max_attention_width) return layer + " is " + std::to_string(o) + " wide, an attention layer at most " + std::to_string(max_attention_width);
            if (o % h) return layer + ": " + std::to_string(h) + " heads do not divide the width " + std::to_string(o);
        }
        if (!(attn_dropout_p >= 0.0 && attn_dropout_p < 1.0)) return "attention dropout probability out of [0, 1)";
        if (variant == 2 && attn_dropout_p != 0.0) return "attention dropout with variant v2, which has none";
        return "";
    }

    // ---- writer ------------------------------------------------------------------------------------------------------
    std::string bytes(const std::string &path_for_errors = "checkpoint") const {
        if (sizes.size() < 2 || sizes.size() > max_sizes) throw checkpoint_error(path_for_errors + ": " + std::to_string(sizes.size()) + " sizes cannot be stored");
        if (model > 1) throw checkpoint_error(path_for_errors + ": model " + std::to_string(model) + " cannot be stored");
        if (model == 1) {
            const auto bad = attention_problem();
            if (!bad.empty()) throw checkpoint_error(path_for_errors + ": " + bad);
        }
        const auto want = expected(sizes, residual_layer, norm, model, variant);
        if (want.size() != tensors.size()) throw checkpoint_error(path_for_errors + ": " + std::to_string(tensors.size()) + " tensors, the configuration has " + std::to_string(want.size()));
        std::string out;
        auto put = [&out](const void *p, std::size_t n) { out.append(static_cast<const char *>(p), n); };
        auto u32 = [&put](std::uint32_t x) { put(&x, 4); };
        auto u64 = [&put](std::uint64_t x) { put(&x, 8); };
        put(magic, 8);
        u32(model == 1 ? version_attention : version), u32((std::uint32_t)sizes.size());
        for (auto s : sizes) u32(s);
        u32(residual_layer ? 1 : 0), u32(norm), u32(loss);
        if (model == 1) {
            u32(model), u32(variant);
            for (auto h : heads) u32(h);
            put(&attn_slope, 8), put(&attn_dropout_p, 8);
        }
        u32(optimizer ? 1 : 0);
        put(&dropout_p, 8);
        u64(dropout_seed), u64(dropout_epoch), u64(optimizer ? step : 0);
        u32((std::uint32_t)tensors.size());
        for (std::size_t k = 0; k < tensors.size(); k++) {
            const auto &t = tensors[k];
            if (t.name != want[k].name || t.rows != want[k].rows || t.cols != want[k].cols || t.data.size() != t.size())
                throw checkpoint_error(path_for_errors + ": tensor " + std::to_string(k) + " is not " + want[k].name + " of the model's shape");
            u32((std::uint32_t)t.name.size());
            put(t.name.data(), t.name.size());
            u32(t.rows), u32(t.cols);
            put(t.data.data(), 4 * t.data.size());
        }
        if (optimizer)
            for (const auto &t : tensors) {
                if (t.m.size() != t.size() || t.v.size() != t.size()) throw checkpoint_error(path_for_errors + ": tensor " + t.name + " has no moments");
                put(t.m.data(), 4 * t.m.size());
                put(t.v.data(), 4 * t.v.size());
            }
        return out;
    }

    void write(const std::string &path) const {
        const std::string b = bytes(path);
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write(b.data(), (std::streamsize)b.size());
        f.close();
        if (!f) throw checkpoint_error(path + ": cannot write");
    }

    // ---- reader ------------------------------------------------------------------------------------------------------
    static checkpoint parse(const std::string &buf, const std::string &path) {
        std::size_t at = 0;
        auto take = [&](void *dst, std::size_t n, const std::string &what) {
            if (n > buf.size() - at)
                throw checkpoint_error(path + ": truncated in " + what + " (needs " + std::to_string(n) + " bytes at offset " + std::to_string(at) + ", the file has " + std::to_string(buf.size()) + ")");
            if (n) std::memcpy(dst, buf.data() + at, n);
            at += n;
        };
        auto u32 = [&](const std::string &what) { std::uint32_t x = 0; take(&x, 4, what); return x; };
        auto u64 = [&](const std::string &what) { std::uint64_t x = 0; take(&x, 8, what); return x; };
        // payload of `count` floats: the length is checked against what is left BEFORE the vector is sized
        auto floats = [&](std::vector<float> &dst, std::size_t count, const std::string &what) {
            if (count > (buf.size() - at) / 4)
                throw checkpoint_error(path + ": truncated in " + what + " (needs " + std::to_string(count) + " floats at offset " + std::to_string(at) + ", the file has " + std::to_string(buf.size()) + " bytes)");
            dst.resize(count);
            take(dst.data(), 4 * count, what);
        };
        checkpoint c;
        char mg[8];
        take(mg, 8, "the magic");
        if (std::memcmp(mg, magic, 8) != 0) throw checkpoint_error(path + ": not a checkpoint file (wrong magic)");
        const auto ver = u32("the version");
        if (ver != version && ver != version_attention)
            throw checkpoint_error(path + ": checkpoint version " + std::to_string(ver) + " is not supported (this reader knows " + std::to_string(version) + " and " + std::to_string(version_attention) + ")");
        const auto L = u32("the layer count");
        if (L < 2 || L > max_sizes) throw checkpoint_error(path + ": " + std::to_string(L) + " sizes");
        for (std::uint32_t i = 0; i < L; i++) {
            c.sizes.push_back(u32("the sizes"));
            if (c.sizes.back() == 0) throw checkpoint_error(path + ": a layer width of zero");
        }
        const auto res = u32("the options"), norm = u32("the options"), loss = u32("the options");
        if (ver == version_attention) {
            c.model = u32("the attention block"), c.variant = u32("the attention block");
            if (c.model != 1) throw checkpoint_error(path + ": unknown model value " + std::to_string(c.model));
            for (std::uint32_t i = 0; i + 1 < L; i++) c.heads.push_back(u32("the heads"));
            take(&c.attn_slope, 8, "the attention block"), take(&c.attn_dropout_p, 8, "the attention block");
            if (res > 1 || norm > 1 || loss > 1) throw checkpoint_error(path + ": unknown option value");
            c.residual_layer = res, c.norm = norm;
            const auto bad = c.attention_problem();
            if (!bad.empty()) throw checkpoint_error(path + ": " + bad);
        }
        const auto opt = u32("the options");
        if (res > 1 || norm > 1 || loss > 1 || opt > 1) throw checkpoint_error(path + ": unknown option value");
        c.residual_layer = res, c.norm = norm, c.loss = loss, c.optimizer = opt;
        take(&c.dropout_p, 8, "the dropout state");
        c.dropout_seed = u64("the dropout state"), c.dropout_epoch = u64("the dropout state"), c.step = u64("the dropout state");
        if (!(c.dropout_p >= 0.0 && c.dropout_p < 1.0)) throw checkpoint_error(path + ": dropout probability out of [0, 1)");
        if (!c.optimizer && c.step) throw checkpoint_error(path + ": a step count without an optimiser section");
        c.tensors = expected(c.sizes, c.residual_layer, c.norm, c.model, c.variant);
        const auto T = u32("the tensor count");
        if (T != c.tensors.size()) throw checkpoint_error(path + ": " + std::to_string(T) + " tensors, the configuration has " + std::to_string(c.tensors.size()));
        for (auto &t : c.tensors) {
            const auto k = u32("the name of " + t.name);
            std::string name(k == t.name.size() ? k : 0, '\0');
            if (k == t.name.size()) take(name.data(), k, "the name of " + t.name);
            if (name != t.name) throw checkpoint_error(path + ": expected tensor " + t.name);
            const auto r = u32("the shape of " + t.name), cl = u32("the shape of " + t.name);
            if (r != t.rows || cl != t.cols) throw checkpoint_error(path + ": tensor " + t.name + " is not " + std::to_string(t.rows) + " x " + std::to_string(t.cols));
            floats(t.data, t.size(), t.name);
        }
        if (c.optimizer)
            for (auto &t : c.tensors) {
                floats(t.m, t.size(), "m." + t.name);
                floats(t.v, t.size(), "v." + t.name);
            }
        if (at != buf.size()) throw checkpoint_error(path + ": " + std::to_string(buf.size() - at) + " trailing bytes");
        return c;
    }

    static checkpoint read(const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw checkpoint_error(path + ": cannot open");
        std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        return parse(buf, path);
    }
};

// Model selection on one monitored number per epoch (the Python twin is selection.model_selector): "improved" is strict --
// lower loss, higher score -- the first best epoch wins a tie and a NaN never improves; stop turns true once `patience`
// epochs (0: never) have passed without improvement.
struct model_selection {
    bool by_score = false;
    std::size_t patience = 0;
    bool has_best = false, stop = false;
    std::size_t best_epoch = 0, since_best = 0;
    double best_value = 0;

    // one epoch's numbers; true when they improved on the best so far
    bool step(std::size_t epoch, double loss, double score) {
        const double value = by_score ? score : loss;
        const bool improved = !std::isnan(value) && (!has_best || (by_score ? value > best_value : value < best_value));
        if (improved) has_best = true, best_epoch = epoch, best_value = value, since_best = 0;
        else since_best++;
        stop = patience > 0 && since_best >= patience;
        return improved;
    }
};

}  // namespace mggcn
