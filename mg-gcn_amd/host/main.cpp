// main.cpp -- the `mg_gcn` command line of the reference (src/main.cpp) on the HIP engine.
//
//   mg_gcn [-h] [-P gpus] [-R 0/1] [-E epochs] [-S x] [-N] train <dir> <k> <h1> ... <hk>
//
// Same flag grammar (getopt "h?P:R:E:S:N", src/main.cpp:58), same dataset files
// (graph.bin / features.bin / labels.bin / sets.bin, :82-85), same stderr lines
// ("n nnz", "num_labels = ", "feature size = ", then per epoch "e loss acc seconds", :87-91,
// :130, :167), same per-epoch timer dump "csvs/<name>_<sizes>_<P>.csv" (:100-111, :131, :168),
// same hyper-parameters (Adam 1e-2 / 0.9 / 0.999 / 5e-4 / 1e-8, :126).  Like the reference,
// P > 1 trains only with -R 1 (row partition); classes are padded to a multiple of P (:135).
// `-R 1` routes through the distributed classes at any P (at -P 1 too: one rank, same schedule).
// Environment: MGGCN_DIST_MODE=allgather|halo|rounds picks the exchange schedule (ops.hpp; rounds = the
// reference's broadcast pipeline); MGGCN_FUSED=0 replays the reference's launch sequence;
// MGGCN_OVERSUBSCRIBE=1 lets -P exceed the visible GPUs (ranks wrap over them, peer-copy transport);
// MGGCN_HOIST_FIRST_AGGREGATION=1 (single GPU) pre-computes the first layer's A.X once (6 SpMMs per epoch: not the
// reference's epoch, same results at 1e-4); MGGCN_AGG_DTYPE=bf16 (single GPU, not -R 1) stores the SpMMs' gathered
// operand in bf16 (f32 or unset: the reference's fp32); MGGCN_TRAIN_SET=0|1|2 trains on that split of sets.bin (0 train /
// 1 validation / 2 test; unset: the reference's loss over all vertices): the epoch line reports the training split and
// a second line, "[mggcn splits] <e> train <loss> <acc> val <loss> <acc> test <loss> <acc>", every split;
// MGGCN_DROPOUT=<p> (single GPU, not -R 1; 0 <= p < 1, unset or 0: none) drops the input of every layer but the first in
// the training forward, with the counter-based mask of mggcn_dropout_f32 for seed MGGCN_DROPOUT_SEED=<u64> (default 0);
// epoch e of the run is dropout epoch e; MGGCN_LAYER_NORM=1 (single GPU, not -R 1; 0 or unset: none) normalises the rows
// of every layer but the last between aggregation / linear and activation (mggcn_layer_norm_forward_f32), gamma and beta
// trained with the weights; MGGCN_LOSS=bce (single GPU, not -R 1; softmax or unset: the reference's loss) trains a
// multi-label model: labels.bin is the n x C target matrix (non-zero = positive), "num_labels = " prints C, the loss is
// sigmoid + binary cross-entropy and the accuracy column of the epoch line and of "[mggcn splits]" holds micro-F1;
// MGGCN_TIMING=1 prints the start-up stages.
// Checkpoints and model selection (all opt-in; with every variable unset nothing changes): MGGCN_LOAD=<file> starts from a
// checkpoint (checkpoint.hpp; the epoch column, the timer prefixes and the dropout epoch continue from its step count, and
// the file's dropout state replaces MGGCN_DROPOUT's); MGGCN_SAVE=<file> writes the full state after the last epoch that ran;
// MGGCN_SAVE_BEST=<file> (needs MGGCN_TRAIN_SET) keeps the parameters of the best validation epoch, by MGGCN_SELECT=loss
// (default) or score, one "[mggcn best] <epoch> <val loss> <val score>" line per improving epoch; MGGCN_PATIENCE=<k> (needs
// MGGCN_TRAIN_SET) stops after k epochs without improvement.  The monitored number is the training forward's own, which
// describes the parameters the epoch STARTED from: those are what is kept.
//
//   mg_gcn -P 1 predict <dir> <k> <h1> ... <hk>
//
// builds the model, loads MGGCN_LOAD, runs one plain forward, writes the int32 predictions ([n x 1] argmax, or [n x C] 0 / 1
// with MGGCN_LOSS=bce) as a dense .bin to MGGCN_PREDICTIONS (default predictions.bin) and prints
// "[mggcn predict] all <score> train <score> val <score> test <score>" from labels.bin and sets.bin.
#include <unistd.h>

#include <chrono>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "gcn.hpp"

using x_t = unsigned;
using v_t = unsigned;
using r_t = float;

class arg_error : public std::runtime_error {
public:
    template <typename T>
    arg_error(T t) : std::runtime_error(t) {}
};

static int usage_(char *prog) {
    std::cout << "Usage: " << prog << " [-h] [-P gpus] [-R 0/1] [-E epochs] [-S x] [-N] train|predict <dir> <k> <h1..hk>" << std::endl;
    return 0;
}

static int help_() {
    std::cout << "\nMG-GCN full-graph multi-GPU GCN training, MI355X (gfx950) engine.\n\n"
                 "Options:\n"
                 "    -P : number of GPUs\n"
                 "    -R : enable the 1D row partition (required for -P > 1)\n"
                 "    -E : number of epochs (default 20)\n"
                 "    -S : disable communication/computation overlap\n"
                 "Environment:\n"
                 "    MGGCN_TRAIN_SET=0|1|2 : train on that split of sets.bin (0 train, 1 validation, 2 test) and report\n"
                 "                            every split per epoch; unset: loss and accuracy over all vertices\n"
                 "    MGGCN_DROPOUT=<p>     : drop the input of every layer but the first with probability p in [0, 1)\n"
                 "                            (single GPU); MGGCN_DROPOUT_SEED=<u64> picks the masks (default 0)\n"
                 "    MGGCN_LAYER_NORM=1    : layer normalisation before the activation of every layer but the last (single GPU)\n"
                 "    MGGCN_LOSS=softmax|bce: bce = multi-label training (single GPU): labels.bin is an n x C 0/1 matrix, the\n"
                 "                            loss sigmoid + binary cross-entropy, the reported score micro-F1\n"
                 "    MGGCN_LOAD=<file>     : start from a checkpoint; epochs and dropout masks continue from its step count\n"
                 "    MGGCN_SAVE=<file>     : write the full state (with Adam's) after the last epoch that ran\n"
                 "    MGGCN_SAVE_BEST=<file>: keep the best validation epoch's parameters (needs MGGCN_TRAIN_SET);\n"
                 "                            MGGCN_SELECT=loss|score picks the monitored number (default loss)\n"
                 "    MGGCN_PATIENCE=<k>    : stop after k epochs without improvement (needs MGGCN_TRAIN_SET)\n"
                 "    MGGCN_PREDICTIONS=<f> : where predict writes (default predictions.bin)\n"
                 "Arguments:\n"
                 "    train <dir> <k> <h1> ... <hk> : dataset directory, number of hidden layers and their widths\n"
                 "    predict <dir> <k> <h1> ... <hk> : load MGGCN_LOAD, one plain forward, predictions as a dense .bin (-P 1)\n";
    return EXIT_SUCCESS;
}

// MGGCN_DUMP_WEIGHTS=<dir>: before every epoch write each layer's W and b as dense .bin files
// (<dir>/e<epoch>_W<layer>.bin, _b<layer>.bin; the reference's own dense format, u32 N, u32 M, f32 payload) so
// that a checker can replay any epoch from the exact state it started in (tests/test_gpu_host_cpp.py).
static void dump_dense(const std::filesystem::path &path, const dn_matrix<float> &A) {
    const auto h = A.to_host();
    std::ofstream out(path, std::ios::binary);
    const std::uint32_t shape[2] = {(std::uint32_t)A.n(), (std::uint32_t)A.m()};
    out.write(reinterpret_cast<const char *>(shape), sizeof shape);
    out.write(reinterpret_cast<const char *>(h.data()), (std::streamsize)(h.size() * sizeof(float)));
}

// MGGCN_TIMING=1: host seconds of every start-up stage on stderr ("[mggcn timing] <stage> <s>"), for the set-up figures
// DESIGN.md quotes; off by default (the reference prints nothing there)
struct stage_timer {
    const bool on = std::getenv("MGGCN_TIMING") && std::string(std::getenv("MGGCN_TIMING")) != "0";
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        const auto now = std::chrono::steady_clock::now();
        if (on) std::cerr << "[mggcn timing] " << what << ' ' << std::chrono::duration<double>(now - last).count() << std::endl;
        last = now;
    }
};

// "[mggcn splits] <e> train <loss> <acc> val <loss> <acc> test <loss> <acc>": every split's pair of the epoch
template <typename metrics_t>
static void print_splits(std::size_t e, const metrics_t &m) {
    std::cerr << "[mggcn splits] " << e << " train " << m[0].first << ' ' << m[0].second << " val " << m[1].first << ' '
              << m[1].second << " test " << m[2].first << ' ' << m[2].second << std::endl;
}

static bool env_is(const char *name, const char *value) {
    const char *s = std::getenv(name);
    return s && std::string(s) == value;
}

// the whole string as a number, or an arg_error naming the variable
static double env_double(const char *name, const std::string &v) {
    std::size_t used = 0;
    double x = 0;
    try { x = std::stod(v, &used); } catch (const std::exception &) { used = 0; }
    if (v.empty() || used != v.size()) throw arg_error(std::string(name) + " must be a number, not '" + v + "'");
    return x;
}
static std::uint64_t env_u64(const char *name, const std::string &v) {
    std::size_t used = 0;
    unsigned long long x = 0;
    try { x = std::stoull(v, &used, 0); } catch (const std::exception &) { used = 0; }
    if (v.empty() || v[0] == '-' || used != v.size()) throw arg_error(std::string(name) + " must be an unsigned 64-bit integer, not '" + v + "'");
    return (std::uint64_t)x;
}

// a path from the environment: unset is empty, set must not be empty
static std::string env_path(const char *name) {
    const char *s = std::getenv(name);
    if (s && !*s) throw arg_error(std::string(name) + " must name a file, not ''");
    return s ? s : "";
}

// `mg_gcn predict`: one plain forward of the loaded model; the predictions as a dense int32 .bin and one score line --
// accuracy, or micro-F1 with MGGCN_LOSS=bce -- over all vertices and per split (nan for an empty split)
template <typename model_t>
static void run_predict(context ctx, model_t &G, dn_matrix<r_t> X, const dn_matrix<std::int32_t> &Y, const dn_matrix<std::int32_t> &S,
                        bool bce, const std::string &out_path) {
    auto H = G(ctx, X);
    const std::size_t n = H.n(), C = H.m(), cols = bce ? C : 1;
    std::vector<std::int32_t> pred;
    if (bce) {
        const auto logits = H.to_host();
        pred.resize(logits.size());
        for (std::size_t i = 0; i < logits.size(); i++) pred[i] = logits[i] > 0 ? 1 : 0;
    } else {
        dn_matrix<std::int32_t> P(n, 1);
        max_row_indices(ctx, H, P);          // the first maximum wins
        ctx.sync();
        pred = P.to_host();
    }
    {
        std::ofstream out(out_path, std::ios::binary);
        const std::uint32_t shape[2] = {(std::uint32_t)n, (std::uint32_t)cols};
        out.write(reinterpret_cast<const char *>(shape), sizeof shape);
        out.write(reinterpret_cast<const char *>(pred.data()), (std::streamsize)(pred.size() * sizeof(std::int32_t)));
        out.close();
        if (!out) throw std::runtime_error(out_path + ": cannot write");
    }
    const auto y = Y.to_host(), sets = S.to_host();
    auto score = [&](int set) {              // set < 0: every vertex
        double hit = 0, rows = 0, tp = 0, fp = 0, fn = 0;
        for (std::size_t i = 0; i < n; i++) {
            if (set >= 0 && sets[i] != set) continue;
            rows += 1;
            if (!bce) { hit += pred[i] == y[i]; continue; }
            for (std::size_t c = 0; c < C; c++) {
                const bool p = pred[i * C + c] != 0, t = y[i * C + c] != 0;
                tp += p && t, fp += p && !t, fn += !p && t;
            }
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (bce) return 2 * tp + fp + fn > 0 ? 2 * tp / (2 * tp + fp + fn) : nan;
        return rows > 0 ? hit / rows : nan;
    };
    std::cerr << "[mggcn predict] all " << score(-1) << " train " << score(0) << " val " << score(1) << " test " << score(2) << std::endl;
}

int main_(int argc, char **argv) {
    opterr = 0;
    std::size_t P = 1, row_partition = 0, num_epochs = 20;
    bool overlap = true;
    while (optind < argc) {
        int c = getopt(argc, argv, "h?P:R:E:S:N");
        if (c == -1) break;
        switch (c) {
            case '?': return usage_(argv[0]);
            case 'h': usage_(argv[0]); return help_();
            case 'P': P = std::stoull(optarg); break;
            case 'R': row_partition = std::stoull(optarg); break;
            case 'E': num_epochs = std::stoull(optarg); break;
            case 'S': overlap = false; break;
            case 'N': overlap = true; break;                       // no_wait: parsed, unused (reference :67)
            default: throw arg_error("Unknown argument.");
        }
    }
    const bool fused = !env_is("MGGCN_FUSED", "0");
    const char *mode_env = std::getenv("MGGCN_DIST_MODE");
    const dist_mode mode = dist_mode_from_string(mode_env ? mode_env : "");
    const bool oversubscribe = std::getenv("MGGCN_OVERSUBSCRIBE") && !env_is("MGGCN_OVERSUBSCRIBE", "0");
    const char *agg_env = std::getenv("MGGCN_AGG_DTYPE");
    const agg_dtype agg = agg_dtype_from_string(agg_env ? agg_env : "");
    if (agg != agg_dtype::f32 && (P > 1 || row_partition))          // the distributed classes have no bf16 aggregation
        throw arg_error("MGGCN_AGG_DTYPE=bf16 is single-GPU only (not with -P > 1 or -R 1)");
    int train_set = -1;                                             // MGGCN_TRAIN_SET unset: the loss over all vertices
    if (const char *ts = std::getenv("MGGCN_TRAIN_SET")) {
        const std::string v = ts;
        if (v != "0" && v != "1" && v != "2") throw arg_error("MGGCN_TRAIN_SET must be 0 (train), 1 (validation) or 2 (test), not '" + v + "'");
        train_set = v[0] - '0';
    }
    double dropout_p = 0;                                           // MGGCN_DROPOUT unset: no dropout, nothing launched
    std::uint64_t dropout_seed = 0;
    if (const char *dp = std::getenv("MGGCN_DROPOUT")) {
        dropout_p = env_double("MGGCN_DROPOUT", dp);
        if (!(dropout_p >= 0.0 && dropout_p < 1.0)) throw arg_error("MGGCN_DROPOUT must be in [0, 1), not '" + std::string(dp) + "'");
        if (dropout_p > 0.0 && (P > 1 || row_partition))            // the distributed classes have no dropout
            throw arg_error("MGGCN_DROPOUT is single-GPU only (not with -P > 1 or -R 1)");
    }
    if (const char *sd = std::getenv("MGGCN_DROPOUT_SEED")) dropout_seed = env_u64("MGGCN_DROPOUT_SEED", sd);
    bool layer_norm_on = false;                                     // MGGCN_LAYER_NORM unset or 0: no norm, nothing launched
    if (const char *ln = std::getenv("MGGCN_LAYER_NORM")) {
        const std::string v = ln;
        if (v != "0" && v != "1") throw arg_error("MGGCN_LAYER_NORM must be 0 or 1, not '" + v + "'");
        layer_norm_on = v == "1";
        if (layer_norm_on && (P > 1 || row_partition))              // the distributed classes have no norm
            throw arg_error("MGGCN_LAYER_NORM is single-GPU only (not with -P > 1 or -R 1)");
    }
    bool loss_bce = false;                                          // MGGCN_LOSS unset or softmax: the reference's loss
    if (const char *ls = std::getenv("MGGCN_LOSS")) {
        const std::string v = ls;
        if (v != "softmax" && v != "bce") throw arg_error("MGGCN_LOSS must be softmax or bce, not '" + v + "'");
        loss_bce = v == "bce";
        if (loss_bce && (P > 1 || row_partition))                   // the distributed classes have no multi-label loss
            throw arg_error("MGGCN_LOSS=bce is single-GPU only (not with -P > 1 or -R 1)");
    }
    // checkpoints and model selection: everything unset is today's run, line for line
    const std::string load_path = env_path("MGGCN_LOAD"), save_path = env_path("MGGCN_SAVE"), best_path = env_path("MGGCN_SAVE_BEST");
    const std::string pred_env = env_path("MGGCN_PREDICTIONS");
    mggcn::model_selection selection;
    if (const char *sl = std::getenv("MGGCN_SELECT")) {
        const std::string v = sl;
        if (v != "loss" && v != "score") throw arg_error("MGGCN_SELECT must be loss or score, not '" + v + "'");
        selection.by_score = v == "score";
        if (train_set < 0) throw arg_error("MGGCN_SELECT needs MGGCN_TRAIN_SET");
    }
    if (const char *pt = std::getenv("MGGCN_PATIENCE")) {
        const std::string v = pt;
        std::size_t used = 0;
        unsigned long long k = 0;
        try { k = std::stoull(v, &used, 10); } catch (const std::exception &) { used = 0; }
        if (v.empty() || v[0] == '-' || v[0] == '+' || used != v.size() || k == 0)
            throw arg_error("MGGCN_PATIENCE must be a positive integer, not '" + v + "'");
        selection.patience = (std::size_t)k;
        if (train_set < 0) throw arg_error("MGGCN_PATIENCE needs MGGCN_TRAIN_SET");
    }
    if (!best_path.empty() && train_set < 0) throw arg_error("MGGCN_SAVE_BEST needs MGGCN_TRAIN_SET");
    const bool selecting = !best_path.empty() || selection.patience > 0;

    while (optind < argc && argv[optind] != nullptr) {
        const std::string command = argv[optind++];
        const bool predicting = command == "predict";
        if (!predicting && command.rfind("train", 0) != 0) throw arg_error("Unknown command.");
        if (predicting && load_path.empty()) throw arg_error("predict needs MGGCN_LOAD");
        if (predicting && (P > 1 || row_partition)) throw arg_error("predict is single-GPU only (not with -P > 1 or -R 1)");
        if (optind >= argc) throw arg_error(command + " needs a dataset directory.");
        const std::filesystem::path dir = argv[optind++];
        if ((int)mggcn_device_count() < (int)std::max<std::size_t>(P, 1) && !(oversubscribe && mggcn_device_count() > 0))
            throw arg_error("not enough GPUs visible for -P");

        stage_timer stage;
        mggcn_set_device(0);
        stage("device");
        csr_matrix<x_t, v_t, r_t> A(dir / "graph.bin");
        dn_matrix<r_t> X(dir / "features.bin");
        dn_matrix<std::int32_t> Y(dir / "labels.bin");
        dn_matrix<std::int32_t> S(dir / "sets.bin");               // loaded, never used (reference :85) -- unless MGGCN_TRAIN_SET
        stage("load-files");
        std::cerr << A.n() << ' ' << A.nnz() << std::endl;
        const auto labels = Y.to_host();
        // MGGCN_LOSS=bce: one logit per column of the target matrix
        const auto num_labels = loss_bce ? (std::int32_t)Y.m() : 1 + *std::max_element(labels.begin(), labels.end());
        std::cerr << "num_labels = " << num_labels << std::endl;
        std::cerr << "feature size = " << X.m() << std::endl;

        if (optind >= argc) throw arg_error("train needs the number of hidden layers.");
        const int num_sizes = std::stoi(argv[optind++]);
        std::vector<std::size_t> sizes{X.m()};
        for (int i = 0; i < num_sizes; i++) {
            if (optind >= argc) throw arg_error("missing hidden layer width.");
            sizes.push_back(std::stoull(argv[optind++]));
        }
        sizes.push_back((std::size_t)num_labels);
        if (loss_bce && Y.m() != sizes.back())
            throw arg_error("MGGCN_LOSS=bce: labels.bin has " + std::to_string(Y.m()) + " columns, the last layer " + std::to_string(sizes.back()));

        // csvs/<[permuted_]name>_<sizes>_<P>.csv (reference :100-111)
        std::string filename;
        bool permuted = false;
        for (const auto &part : (dir / "graph.bin").parent_path()) {
            if (part == "permuted") permuted = true;
            else if (!part.empty() && part != "/" && part != ".") filename = (permuted ? std::string("permuted_") : std::string("")) + part.string();
        }
        for (auto s : sizes) filename += "_" + std::to_string(s);
        std::ofstream of;                                            // predict times nothing
        if (!predicting) {
            std::filesystem::create_directories("csvs");
            of.open("csvs/" + filename + "_" + std::to_string(P) + ".csv");
        }
        mggcn::checkpoint candidate;                                 // selection: the parameters the running epoch started from

        if (P <= 1 && !row_partition) {
            auto ctx = context(0);
            gcn<x_t, v_t, r_t> G(A, sizes, false, fused, agg);
            if (env_is("MGGCN_HOIST_FIRST_AGGREGATION", "1")) G.set_hoist_first_aggregation(true);   // optional 6-SpMM epoch
            if (train_set >= 0) G.set_splits(S, train_set);
            if (dropout_p > 0.0) G.set_dropout(dropout_p, dropout_seed);             // train_forward number e is dropout epoch e
            if (layer_norm_on) G.set_layer_norm(true);
            if (loss_bce) G.set_loss_bce();
            std::size_t first_epoch = 0;
            if (!load_path.empty()) {                                 // a configuration mismatch ends the run here
                G.load(ctx, load_path);
                first_epoch = G.adam_steps();
            }
            ctx.sync();
            stage("model (normalize, transpose, layers)");
            if (predicting) {
                run_predict(ctx, G, X, Y, S, loss_bce, pred_env.empty() ? std::string("predictions.bin") : pred_env);
                continue;
            }
            ctx.record("training-start", 0);
            for (std::size_t e = first_epoch; e < first_epoch + num_epochs; e++) {
                if (const char *dd = std::getenv("MGGCN_DUMP_WEIGHTS")) {
                    std::filesystem::create_directories(dd);
                    for (std::size_t l = 0; l < G.layers().size(); l++) {
                        dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_W" + std::to_string(l) + ".bin"), G.layers()[l].W());
                        dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_b" + std::to_string(l) + ".bin"), G.layers()[l].b());
                        if (auto *nm = G.layers()[l].layer_norm_params()) {     // MGGCN_LAYER_NORM=1: _gamma<layer>.bin, _beta<layer>.bin too
                            dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_gamma" + std::to_string(l) + ".bin"), nm->gamma);
                            dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_beta" + std::to_string(l) + ".bin"), nm->beta);
                        }
                    }
                }
                if (selecting) candidate = G.state(ctx, false);
                const auto start = std::chrono::system_clock::now();
                auto [loss, acc] = G.train_forward(ctx, X, Y);
                G.backward(ctx);
                G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8);
                ctx.sync();
                const auto duration = std::chrono::duration<double>{std::chrono::system_clock::now() - start}.count();
                std::cerr << e << ' ' << loss << ' ' << acc << ' ' << duration << std::endl;
                if (train_set >= 0) print_splits(e, G.split_metrics());
                if (e == first_epoch) stage("epoch 0 (SpMM plans built on first use)");
                ctx.dump_timers(of, std::to_string(e) + "_0_");
                if (selecting) {
                    const auto m = G.split_metrics();
                    if (selection.step(e, m[1].first, m[1].second)) {
                        std::cerr << "[mggcn best] " << e << ' ' << m[1].first << ' ' << m[1].second << std::endl;
                        if (!best_path.empty()) candidate.write(best_path);
                    }
                    if (selection.stop) break;
                }
            }
            if (!save_path.empty()) G.save(ctx, save_path);
        } else if (row_partition) {
            sizes.back() = (sizes.back() + P - 1) / P * P;          // reference :135
            auto ctx = dist_context(P, overlap);
            std::vector<v_t> p(P + 1);
            for (std::size_t i = 1; i < p.size(); i++) p[i] = (v_t)(i * A.n() / P);
            stage("dist_context");
            if (stage.on) std::cerr << "[mggcn timing] transport " << ctx.transport() << " enqueue-threads " << (int)ctx.threaded() << std::endl;
            A.normalize(true);
            auto A_T = A.transpose();
            stage("normalize + transpose");
            dist_row_dn_matrix<std::int32_t> Yd(ctx, Y);
            dist_row_csr_matrix<x_t, v_t, r_t> Ad(ctx, A, p, p);
            dist_row_csr_matrix<x_t, v_t, r_t> A_Td(ctx, A_T, p, p);
            stage("block split (A, A_T)");
            dist_gcn<true, x_t, v_t, r_t> G(ctx, Ad, A_Td, sizes, false, fused, mode);
            dist_row_dn_matrix<r_t> Xd(ctx, X);
            if (train_set >= 0) G.set_splits(ctx, dist_row_dn_matrix<std::int32_t>(ctx, S), train_set);
            std::size_t first_epoch = 0;
            if (!load_path.empty()) {                                 // every replica; a configuration mismatch ends the run here
                G.load(ctx, load_path);
                first_epoch = G.adam_steps();
            }
            ctx.sync();
            stage("model + shards");
            ctx.record("training-start", 0);
            for (std::size_t e = first_epoch; e < first_epoch + num_epochs; e++) {
                if (const char *dd = std::getenv("MGGCN_DUMP_WEIGHTS")) {     // GPU 0's replica: they are all the same
                    ctx.sync();
                    std::filesystem::create_directories(dd);
                    for (std::size_t l = 0; l < G.layers().size(); l++) {
                        dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_W" + std::to_string(l) + ".bin"), G.layers()[l].W()[0]);
                        dump_dense(std::filesystem::path(dd) / ("e" + std::to_string(e) + "_b" + std::to_string(l) + ".bin"), G.layers()[l].b()[0]);
                    }
                }
                if (selecting) candidate = G.state(ctx, false);       // GPU 0's replica
                const auto start = std::chrono::system_clock::now();
                const double waited = ctx.device_wait_seconds();
                auto [loss, acc] = G.train_forward(ctx, Xd, Yd);
                G.backward(ctx);
                G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8);
                ctx.sync();
                const auto duration = std::chrono::duration<double>{std::chrono::system_clock::now() - start}.count();
                std::cerr << e << ' ' << loss << ' ' << acc << ' ' << duration << "\n";
                if (train_set >= 0) print_splits(e, G.split_metrics());
                // how much of the epoch the host needed to ISSUE it (wall time minus the time it sat waiting for the devices)
                if (stage.on) std::cerr << "[mggcn timing] epoch " << e << " host-issue-ms " << (duration - (ctx.device_wait_seconds() - waited)) * 1e3 << std::endl;
                if (e == first_epoch) stage("epoch 0 (exchange forms + SpMM plans built on first use)");
                ctx.dump_timers(of, std::to_string(e) + "_");
                if (selecting) {
                    const auto m = G.split_metrics();
                    if (selection.step(e, m[1].first, m[1].second)) {
                        std::cerr << "[mggcn best] " << e << ' ' << m[1].first << ' ' << m[1].second << std::endl;
                        if (!best_path.empty()) candidate.write(best_path);
                    }
                    if (selection.stop) break;
                }
            }
            if (!save_path.empty()) G.save(ctx, save_path);
        }
        // P > 1 without -R 1 trains nothing, exactly like the reference (:145, :171-189)
    }
    return EXIT_SUCCESS;
}

int main(int argc, char **argv) {
    try {
        return main_(argc, argv);
    } catch (const std::exception &e) {
        std::cerr << "Error: uncaught exception: '" << e.what() << "' Aborting." << std::endl;
        std::exit(EXIT_FAILURE);
    }
}
