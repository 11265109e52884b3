// azr_host.cpp — implementation of the reference-shaped host classes over the C-ABI (see azr_host.hpp).
#include "azr_host.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <map>
#include <random>
#include <sstream>

namespace azrhost {

Settings SETTINGS;

// ---- Settings ---------------------------------------------------------------------------------------------------
namespace {
// How a flag's value reaches its Settings member.  TEXT: read by name in Settings::init (the reference's flags, parsed with bare atoi /
// atof as the reference does, and the flags with rules of their own).  The other kinds are parsed, range-checked and assigned by one
// loop, in table order: REAL lo <= v <= hi (lo_open: lo < v), WHOLE the same over whole numbers, SWITCH 0 or 1, SEED a whole number in
// [0, 2^32 - 1], SEED_UNCHECKED whatever strtoul makes of the text (--seed, --dir-seed, --cap-seed: as they always were).
enum Kind { TEXT, REAL, WHOLE, SWITCH, SEED, SEED_UNCHECKED };
struct Opt {
    const char* name; const char* desc; std::string def; bool is_bool;
    Kind kind = TEXT;
    float Settings::*f = nullptr; int Settings::*i = nullptr; uint32_t Settings::*u = nullptr;   // the member it fills: the one of its kind
    double lo = 0, hi = 0; bool lo_open = false;
    const char* what = "";      // the tail of "--name: 'value' ..." when the value is refused
    bool after_next = false;    // checked after the row below it (--resign-streak is checked before --resign-q)
};
Opt real(const char* name, const char* desc, const char* def, float Settings::*m, double lo, double hi, const char* what, bool lo_open = false, bool after_next = false)
{
    return {name, desc, def, false, REAL, m, nullptr, nullptr, lo, hi, lo_open, what, after_next};
}
Opt whole(const char* name, const char* desc, const char* def, int Settings::*m, double lo, double hi, const char* what)
{
    return {name, desc, def, false, WHOLE, nullptr, m, nullptr, lo, hi, false, what};
}
Opt onoff(const char* name, const char* desc, const char* def, int Settings::*m)
{
    return {name, desc, def, false, SWITCH, nullptr, m, nullptr, 0, 1, false, "is neither 0 nor 1"};
}
Opt seed(const char* name, const char* desc, const std::string& def, uint32_t Settings::*m, Kind kind)
{
    return {name, desc, def, false, kind, nullptr, nullptr, m, 0, 0, false, "is not a 32-bit seed"};
}

bool parse_bool(const std::string& v) { return !(v == "0" || v == "false" || v == "False" || v == "no"); }

void mkdirs(const std::string& path)
{
    std::string cur;
    for (size_t i = 0; i < path.size(); i++) {
        cur += path[i];
        if (path[i] == '/' || i + 1 == path.size()) mkdir(cur.c_str(), 0777);
    }
}
}  // namespace

// One host thread per GPU (the reference's structure: alphazero_trainer.cpp:48-57, game.cpp:277-312).  An exception thrown in a
// thread body would end the process in std::terminate: it is caught there, every thread is joined, and the first failure is
// raised in the caller's thread with the GPU it came from.
void forEachGpu(int P, const char* what, const std::function<void(int)>& body)
{
    std::vector<std::string> failed(P);
    std::vector<std::thread> threads;
    for (int i = 0; i < P; i++)
        threads.emplace_back([&, i]() {
            try { body(i); }
            catch (const std::exception& ex) { failed[i] = ex.what()[0] ? ex.what() : "unknown error"; }
            catch (...) { failed[i] = "unknown error"; }
        });
    for (auto& t : threads) t.join();
    for (int i = 0; i < P; i++)
        if (!failed[i].empty()) throw std::runtime_error(std::string(what) + " on gpu " + std::to_string(i) + ": " + failed[i]);
}

void Settings::init(int argc, char* argv[])
{
    // name, description (as the reference's help text), default — settings.h:91-137
    std::vector<Opt> opts = {
        {"m", "Mode [train/play]", MODE, false},
        {"g", "Default graph file path", DEFAULT_GRAPH_DEF_PB, false},
        {"c", "Checkpoint file path", DEFAULT_LATEST_CHECKPOINT, false},
        {"p1", "Player 1 [az/sp]", PLAYER_1, false},
        {"g1", "Graph file path for player 1", GRAPH_DEF_PB_1, false},
        {"c1", "Checkpoint file path for player 1", CHECKPOINT_1, false},
        {"p2", "Player 2 [az/sp]", PLAYER_2, false},
        {"g2", "Graph file path for player 2", GRAPH_DEF_PB_2, false},
        {"c2", "Checkpoint file path for player 2", CHECKPOINT_2, false},
        {"gpus", "Number of gpu units", std::to_string(NUMBER_OF_GPUS), false},
        {"gpu-games", "Number of concurent games per gpu", std::to_string(NUMBER_OF_CONCURENT_GAMES_PER_GPU), false},
        {"t", "Number of threads", std::to_string(THREADS_PER_MCTS), false},
        {"apbs", "Set number of games per gpu to get avg. prediction batch size", std::to_string(AVG_PRED_BATCH_SIZE), false},
        {"lnt", "Log nn training", std::to_string(LOG_NN_TRAINING), true},
        {"ls", "Log state", std::to_string(LOG_STATE), true},
        {"dgss", "Number of data games for trin-data script vs script", std::to_string(DATA_GAMES_SS), false},
        {"dgsr", "Number of data games for trin-data script vs random", std::to_string(DATA_GAMES_SR), false},
        {"dtl", "Number of train loops for data games", std::to_string(DATA_TRAIN_LOOPS), false},
        {"allow-yield", "Allow yield when enemy ownes 3/4 of lands", std::to_string(ALLOW_YIELD), true},
        {"limit-reinforcement", "Limit reinforcement moves", std::to_string(LIMIT_REINFORCEMENT_MOVES), true},
        {"limit-attack", "Limit attack moves", std::to_string(LIMIT_ATTACK_MOVES), true},
        {"mirror-games", "Play games in pair with mirrored initial position", std::to_string(MIRROR_GAMES), true},
        {"ti", "Number of train iterations", std::to_string(TRAIN_ITERATIONS), false},
        {"tg", "Games played per train iteration", std::to_string(TRAIN_ITERATION_GAMES), false},
        {"mcts", "Number of MCTS simulations", std::to_string(MCTS_SIMULATIONS), false},
        {"hp", "Exploration factor", std::to_string(HP_EXPLORATION), false},
        {"dnv", "Dirchlet noise value", std::to_string(DIR_NOISE_VALUE), false},
        {"dne", "Dirchlet noise epsi", std::to_string(DIR_NOISE_EPSI), false},
        {"temp", "Temperature trehsold", std::to_string(TEMPERATURE_TRESHOLD), false},
        {"e", "Number of epochs per train iteration", std::to_string(EPOCHS), false},
        {"bs", "Batch size", std::to_string(BATCH_SIZE), false},
        {"cg", "Number of games for comparison", std::to_string(COMPARE_GAMES), false},
        {"ct", "Treshold for accepted improvement", std::to_string(COMPARE_TRESHOLD), false},
        {"s", "Number of stored samples", std::to_string(SAMPLES_STORAGE_MIN), false},
        {"blocks", "[this build] residual blocks of the net (reference: compile-time BLOCKS)", std::to_string(BLOCKS), false},
        {"dtype", "[this build] net arithmetic bf16|f16|f32x|f32 (f32x = fp32-equivalent on the MFMA)", NET_DTYPE, false},
        {"blocks2", "[this build] residual blocks of player 2's net in -m play --p1 az --p2 az (if not --blocks, --c2 defaults to checkpoints/latest-checkpoint-N-blocks.bin)", "--blocks", false},
        {"dtype2", "[this build] arithmetic of player 2's net in -m play --p1 az --p2 az", "--dtype", false},
        {"mcts2", "[this build] MCTS simulations of player 2 in -m play --p1 az --p2 az (a search budget per side)", "--mcts", false},
        {"hp2", "[this build] exploration factor of player 2 in -m play --p1 az --p2 az", "--hp", false},
        seed("seed", "[this build] base seed of the per-game RNG streams", std::to_string(BASE_SEED), &Settings::BASE_SEED, SEED_UNCHECKED),
        {"devices", "[this build] HIP device of every logical gpu, comma separated (default 0,1,..; \"0,0\" rehearses --gpus 2 on one card)", "", false},
        {"pair-halves", "[this build] mirrored pairs: 1 = both games of a pair at the same time on two slots, 0 = one after the other on one slot", std::to_string(CONCURRENT_PAIR_HALVES), true},
        real("dir-alpha", "[this build] self-play root noise: Dirichlet(alpha) over the root's legal moves, drawn per decision (0 = the reference's constant --dnv; at most 10)", "0", &Settings::DIR_ALPHA, 0, 10, "is not a Dirichlet parameter (0 = off, at most 10)"),
        seed("dir-seed", "[this build] seed of the self-play root noise (independent of --seed: the games' dice and deals do not move)", std::to_string(DIR_SEED), &Settings::DIR_SEED, SEED_UNCHECKED),
        real("cap-prob", "[this build] self-play playout cap: share of decisions that get the whole --mcts search, root noise and a training record; the others search --cap-fast simulations and write none (1 = off: every decision)", "1", &Settings::CAP_PROB, 0, 1, "is not a probability (a number in [0, 1]; 1 = off)"),
        whole("cap-fast", "[this build] simulations of a fast decision under --cap-prob (0 = off; else within [-t, --mcts])", "0", &Settings::CAP_FAST, 0, HUGE_VAL, "is not a simulation count (0 = off)"),
        seed("cap-seed", "[this build] seed of the playout cap's coin (independent of --seed and --dir-seed: dice, deals and noise do not move)", std::to_string(CAP_SEED), &Settings::CAP_SEED, SEED_UNCHECKED),
        real("forced-k", "[this build] self-play forced playouts: a tried root move of a full decision is searched until it has sqrt(k * prior * visits) visits (0 = off; at most 8; KataGo runs 2)", "0", &Settings::FORCED_K, 0, 8, "is not a forced-playout factor (a number in [0, 8]; 0 = off)"),
        onoff("prune-target", "[this build] self-play policy target pruning under --forced-k: 1 = the recorded pi leaves out the forced visits PUCT would not have spent (0 = off)", "0", &Settings::PRUNE_TARGET),
        real("psw-share", "[this build] self-play policy surprise weighting: share of a finished game's record weight handed out in proportion to KL(recorded pi || net prior); a record is then written floor(w) or ceil(w) times (0 = off: every record once; at most 1; KataGo runs 0.5)", "0", &Settings::PSW_SHARE, 0, 1, "is not a share (a number in [0, 1]; 0 = off)"),
        real("psw-max", "[this build] cap on one record's weight under --psw-share (within [1, 64])", "4", &Settings::PSW_MAX, 1, 64, "is not a weight cap (a number in [1, 64])"),
        seed("psw-seed", "[this build] seed of the coin that rounds a record's weight to its copy count (independent of --seed, --dir-seed and --cap-seed)", std::to_string(PSW_SEED), &Settings::PSW_SEED, SEED),
        real("q-share", "[this build] self-play value mix: share of the search's root value q in the records' value target, z' = (1 - share) * z + share * q (0 = off: the bare game outcome; at most 1; Lc0's q_ratio)", "0", &Settings::Q_SHARE, 0, 1, "is not a share (a number in [0, 1]; 0 = off)"),
        real("resign-q", "[this build] self-play resignation: the bound on the search's root value q; a player whose q stays below it for --resign-streak of its own recorded decisions in a row gives the game up (within [-1, 1]; AlphaGo Zero, KataGo)", "-0.9", &Settings::RESIGN_Q, -1, 1, "is not a bound on the root value (a number in [-1, 1])", false, true),
        whole("resign-streak", "[this build] decisions in a row below --resign-q after which their player resigns (0 = off: every game is played to its end; at most 255)", "0", &Settings::RESIGN_STREAK, 0, 255, "is not a streak (a whole number in [0, 255]; 0 = off)"),
        real("resign-holdout", "[this build] share of the self-play games that never resign and report how often the would-be resigner did not lose (within [0, 1])", "0.1", &Settings::RESIGN_HOLDOUT, 0, 1, "is not a share (a number in [0, 1])"),
        seed("resign-seed", "[this build] seed of the coin that holds a game out of resignation (independent of --seed, --dir-seed, --cap-seed and --psw-seed)", std::to_string(RESIGN_SEED), &Settings::RESIGN_SEED, SEED),
        whole("gumbel-m", "[this build] self-play Gumbel root search with sequential halving: moves considered at a root, sampled without replacement through Gumbel noise; the winner is played and softmax(logit + sigma(completed Q)) recorded (0 = off: PUCT at the root, the visit distribution as pi; at most 43; not with --dir-alpha, --cap-prob or --forced-k; Danihelka et al. 2022)", "0", &Settings::GUMBEL_M, 0, 43, "is not a number of root moves (a whole number in [0, 43]; 0 = off)"),
        real("gumbel-cvisit", "[this build] c_visit of sigma = ((c_visit + max N) * c_scale) * completed Q under --gumbel-m (at least 0)", "50", &Settings::GUMBEL_CVISIT, 0, 1e30, "is not a c_visit (a finite number, at least 0)"),
        real("gumbel-cscale", "[this build] c_scale of sigma under --gumbel-m, for values in [-1, 1]: half the paper's, whose values lie in [0, 1] (above 0)", "0.5", &Settings::GUMBEL_CSCALE, 0, 1e30, "is not a c_scale (a finite number above 0)", true),
        seed("gumbel-seed", "[this build] seed of the Gumbel vectors (independent of --seed: the games' dice and deals do not move)", std::to_string(GUMBEL_SEED), &Settings::GUMBEL_SEED, SEED),
        onoff("gumbel-tree", "[this build] under --gumbel-m, the selection below the root: 1 = every interior node spends its visits in proportion to softmax(logit + sigma(completed Q)) of its own rows, the paper's full search (0 = PUCT there)", "0", &Settings::GUMBEL_TREE),
        whole("arena-gumbel-m", "[this build] arena games (compare and benchmark games of -m learn, -m play): Gumbel search with sequential halving of player 1 — the new net of the compare games, the AlphaZero side against Script and Random — over this many root moves, deterministic (no Gumbel noise), c_visit and c_scale of --gumbel-cvisit / --gumbel-cscale (0 = off: PUCT; at most 43)", "0", &Settings::ARENA_GUMBEL_M, 0, 43, "is not a number of root moves (a whole number in [0, 43]; 0 = off)"),
        whole("arena-gumbel-m2", "[this build] the same for player 2, the old net of the compare games and player 2 of -m play --p1 az --p2 az (not given: the value of --arena-gumbel-m)", "0", &Settings::ARENA_GUMBEL_M2, 0, 43, "is not a number of root moves (a whole number in [0, 43]; 0 = off)"),
        onoff("arena-gumbel-tree", "[this build] under --arena-gumbel-m, player 1's selection below the root: 1 = by the improved policy of each node (0 = PUCT there)", "0", &Settings::ARENA_GUMBEL_TREE),
        onoff("arena-gumbel-tree2", "[this build] under --arena-gumbel-m2, the same for player 2 (not given: the value of --arena-gumbel-tree)", "0", &Settings::ARENA_GUMBEL_TREE2),
        {"cvk", "[this build] folds of -m analysis (the reference hard-codes 10)", std::to_string(CV_K), false},
        {"cv-max-epochs", "[this build] cap on the epochs of one -m analysis fold (0 = no cap, the reference's loop)", std::to_string(CV_MAX_EPOCHS), false},
        {"help", "Display help", "0", true},
    };
    // the optimiser step's options (azr_nn_train_set_options): a table of their own, next to the one above and not in it; parsed, listed
    // and written to the settings file like its rows, range-checked behind them, then the rules that tie them to --lr-schedule
    const std::vector<Opt> train_opts = {
        real("lr", "[this build] optimiser step: base learning rate (above 0; the reference's graph has 1e-3)", "0.001", &Settings::LR, 0, 1e30, "is not a learning rate (a finite number above 0)", true),
        real("l2", "[this build] optimiser step: L2 coefficient of the conv / dense kernels (at least 0; the reference's graph has 1e-3)", "0.001", &Settings::L2, 0, 1e30, "is not an L2 coefficient (a finite number, at least 0)"),
        {"lr-schedule", "[this build] optimiser step: learning-rate schedule over Adam's step count: constant, cosine (from --lr at --lr-warmup down to --lr-min at --lr-steps) or step (times --lr-gamma every --lr-period steps)", LR_SCHEDULE, false},
        whole("lr-warmup", "[this build] optimiser step: steps of linear warm-up to the scheduled rate (0 = none)", "0", &Settings::LR_WARMUP, 0, 2147483647.0, "is not a number of warm-up steps (a whole number, at least 0)"),
        whole("lr-steps", "[this build] optimiser step: the step at which the cosine schedule reaches --lr-min (above --lr-warmup)", "0", &Settings::LR_STEPS, 0, 2147483647.0, "is not a step count (a whole number, at least 0)"),
        real("lr-min", "[this build] optimiser step: floor of the cosine schedule (within [0, --lr])", "0", &Settings::LR_MIN, 0, 1e30, "is not a learning rate (a finite number, at least 0)"),
        whole("lr-period", "[this build] optimiser step: steps between two decays of the step schedule (at least 1)", "1", &Settings::LR_PERIOD, 1, 2147483647.0, "is not a decay period (a whole number, at least 1)"),
        real("lr-gamma", "[this build] optimiser step: factor of one decay of the step schedule (within (0, 1])", "1", &Settings::LR_GAMMA, 0, 1, "is not a decay factor (a number in (0, 1])", true),
        real("clip-norm", "[this build] optimiser step: the gradient of the whole loss is scaled down to this global norm (tf.clip_by_global_norm; 0 = off)", "0", &Settings::CLIP_NORM, 0, 1e30, "is not a norm to clip to (a finite number above 0; 0 = off)"),
        real("ema-decay", "[this build] optimiser step: decay d of an exponential moving average of the weights, e = d e + (1 - d) w after every step (within (0, 1); 0 = off)", "0", &Settings::EMA_DECAY, 0, 0.99999994, "is not an EMA decay (a number in (0, 1); 0 = off)"),
        onoff("ema-play", "[this build] 1 = the averaged net of --ema-decay plays the compare games, is saved and generates the next games, while training goes on with the raw weights (0 = the raw net does)", "0", &Settings::EMA_PLAY),
    };
    std::map<std::string, std::string> val;
    std::map<std::string, bool> given;
    auto find = [&](const std::string& n) -> const Opt* {
        for (auto& o : opts) if (n == o.name) return &o;
        for (auto& o : train_opts) if (n == o.name) return &o;
        return nullptr;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-h") a = "--help";
        std::string name, value;
        bool has_value = false;
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            if (eq != std::string::npos) { value = a.substr(eq + 1); has_value = true; }
        } else if (a.size() >= 2 && a[0] == '-') {
            name = a.substr(1, 1);  // cxxopts: one-letter names are short options (-m train, -mtrain, -t 1)
            if (a.size() > 2) { value = a.substr(a[2] == '=' ? 3 : 2); has_value = true; }
        } else {
            fprintf(stderr, "unexpected argument '%s'\n", a.c_str());
            exit(2);
        }
        const Opt* o = find(name);
        if (!o) { fprintf(stderr, "Option '%s' does not exist\n", name.c_str()); exit(2); }
        if (!has_value) {
            if (o->is_bool && (i + 1 >= argc || argv[i + 1][0] == '-')) value = "1";
            else if (i + 1 < argc) value = argv[++i];
            else { fprintf(stderr, "Option '%s' is missing an argument\n", name.c_str()); exit(2); }
        }
        val[name] = value;
        given[name] = true;
    }
    auto get = [&](const char* n) { return given.count(n) ? val[n] : find(n)->def; };
    if (given.count("help")) {
        printf("AlphaZero implementation for game Risk (MI355X-native hot path)\nUsage:\n  AlphaZero-Risk [OPTION...]\n\n");
        for (const std::vector<Opt>* t : {(const std::vector<Opt>*)&opts, &train_opts})
            for (auto& o : *t) printf("  %s%-22s %s (default: %s)\n", strlen(o.name) == 1 ? " -" : "--", o.name, o.desc, o.def.c_str());
        exit(0);
    }
    MODE = get("m");
    if (MODE == "learn") MODE = "train";  // BASELINE.json calls the reference's `train` mode `learn`
    DEFAULT_GRAPH_DEF_PB = get("g");
    DEFAULT_LATEST_CHECKPOINT = get("c");
    PLAYER_1 = get("p1"); GRAPH_DEF_PB_1 = get("g1"); CHECKPOINT_1 = get("c1");
    PLAYER_2 = get("p2"); GRAPH_DEF_PB_2 = get("g2"); CHECKPOINT_2 = get("c2");
    THREADS_PER_MCTS = atoi(get("t").c_str());
    NUMBER_OF_GPUS = atoi(get("gpus").c_str());
    if (given.count("gpu-games")) NUMBER_OF_CONCURENT_GAMES_PER_GPU = atoi(get("gpu-games").c_str());
    else NUMBER_OF_CONCURENT_GAMES_PER_GPU = AVG_PRED_BATCH_SIZE / (THREADS_PER_MCTS > 0 ? THREADS_PER_MCTS : 1) * 2;
    DATA_GAMES_SS = atoi(get("dgss").c_str());
    DATA_GAMES_SR = atoi(get("dgsr").c_str());
    DATA_TRAIN_LOOPS = atoi(get("dtl").c_str());
    LOG_STATE = parse_bool(get("ls"));
    ALLOW_YIELD = parse_bool(get("allow-yield"));
    LIMIT_REINFORCEMENT_MOVES = parse_bool(get("limit-reinforcement"));
    LIMIT_ATTACK_MOVES = parse_bool(get("limit-attack"));
    MIRROR_GAMES = parse_bool(get("mirror-games"));
    TRAIN_ITERATIONS = atol(get("ti").c_str());
    TRAIN_ITERATION_GAMES = atoi(get("tg").c_str());
    MCTS_SIMULATIONS = atoi(get("mcts").c_str());
    HP_EXPLORATION = (float)atof(get("hp").c_str());
    DIR_NOISE_VALUE = (float)atof(get("dnv").c_str());
    DIR_NOISE_EPSI = (float)atof(get("dne").c_str());
    TEMPERATURE_TRESHOLD = atoi(get("temp").c_str());
    EPOCHS = atoi(get("e").c_str());
    BATCH_SIZE = atoi(get("bs").c_str());
    COMPARE_GAMES = atoi(get("cg").c_str());
    COMPARE_TRESHOLD = (float)atof(get("ct").c_str());
    SAMPLES_STORAGE_MIN = atoi(get("s").c_str());
    BLOCKS = atoi(get("blocks").c_str());
    NET_DTYPE = get("dtype");
    // player 2's net: what --blocks / --dtype say unless given (the settings file then carries the value in force, not the word "--blocks")
    if (!given.count("blocks2")) val["blocks2"] = get("blocks");
    if (!given.count("dtype2")) val["dtype2"] = get("dtype");
    BLOCKS2 = atoi(val["blocks2"].c_str());
    NET_DTYPE2 = val["dtype2"];
    // A checkpoint holds the fp32 parameters of ONE depth, and --c1 / --c2 default to the same file: a player 2 of another depth whose
    // checkpoint was not named gets a default of its own (a missing checkpoint is initialised and saved, as for every net)
    if (BLOCKS2 != BLOCKS && !given.count("c2")) {
        CHECKPOINT_2 = DEFAULT_CHECKPOINT_DIR + "/latest-checkpoint-" + std::to_string(BLOCKS2) + "-blocks.bin";
        val["c2"] = CHECKPOINT_2;
    }
    if (NET_DTYPE2 != "bf16" && NET_DTYPE2 != "f16" && NET_DTYPE2 != "f32x" && NET_DTYPE2 != "f32") {
        fprintf(stderr, "--dtype2: unknown net arithmetic '%s' (bf16|f16|f32x|f32)\n", NET_DTYPE2.c_str());
        exit(2);
    }
    // player 2's search: what --mcts / --hp say unless given
    SEARCH2_GIVEN = given.count("mcts2") || given.count("hp2");
    if (!given.count("mcts2")) val["mcts2"] = get("mcts");
    if (!given.count("hp2")) val["hp2"] = get("hp");
    {
        char* end = nullptr;
        const long m2 = strtol(val["mcts2"].c_str(), &end, 10);
        if (given.count("mcts2") && (val["mcts2"].empty() || *end != '\0' || m2 < 1 || m2 > 4094)) {
            fprintf(stderr, "--mcts2: '%s' is not a simulation count (1..4094)\n", val["mcts2"].c_str());
            exit(2);
        }
        MCTS_SIMULATIONS2 = (int)m2;
        const int threads = std::max(1, std::min(8, THREADS_PER_MCTS));
        if (given.count("mcts2") && MCTS_SIMULATIONS2 < threads) {   // S - S % T simulations would be none
            fprintf(stderr, "--mcts2: %d simulations are fewer than the %d search threads (-t)\n", MCTS_SIMULATIONS2, threads);
            exit(2);
        }
        const double h2 = strtod(val["hp2"].c_str(), &end);
        if (given.count("hp2") && (val["hp2"].empty() || *end != '\0' || !(h2 >= 0.0))) {
            fprintf(stderr, "--hp2: '%s' is not an exploration factor (a number >= 0)\n", val["hp2"].c_str());
            exit(2);
        }
        HP_EXPLORATION2 = (float)h2;
    }
    CONCURRENT_PAIR_HALVES = parse_bool(get("pair-halves"));
    // the typed rows: parsed, range-checked and assigned in table order; the first value out of range ends the run
    auto fill = [&](const Opt& o) {
        if (o.kind == TEXT) return;
        const std::string v = get(o.name);
        char* end = nullptr;
        bool bad = v.empty();
        if (o.kind == SEED_UNCHECKED) {
            this->*o.u = (uint32_t)strtoul(v.c_str(), nullptr, 10);
            return;
        } else if (o.kind == SEED) {
            const unsigned long long x = bad || v[0] == '-' ? 0 : strtoull(v.c_str(), &end, 10);
            bad = bad || v[0] == '-' || *end != '\0' || x > 0xffffffffull;
            if (!bad) this->*o.u = (uint32_t)x;
        } else if (o.kind == REAL) {
            const double x = strtod(v.c_str(), &end);
            bad = bad || *end != '\0' || !(o.lo_open ? x > o.lo : x >= o.lo) || !(x <= o.hi);   // (a NaN fails)
            if (!bad) this->*o.f = (float)x;
        } else {   // WHOLE, SWITCH
            const long x = strtol(v.c_str(), &end, 10);
            bad = bad || *end != '\0' || (double)x < o.lo || (double)x > o.hi;
            if (!bad) this->*o.i = (int)x;
        }
        if (bad) {
            fprintf(stderr, "--%s: '%s' %s\n", o.name, v.c_str(), o.what);
            exit(2);
        }
    };
    size_t row = 0;
    auto fill_through = [&](const char* last) {   // from where the previous call stopped to the row named `last` (none: to the end)
        for (bool more = true; more && row < opts.size(); row++) {
            if (opts[row].after_next) { fill(opts[row + 1]); fill(opts[row]); row++; }   // (never the two last rows of a call)
            else fill(opts[row]);
            more = strcmp(opts[row].name, last) != 0;
        }
    };
    // the rules between flags, where they always stood among the range checks
    fill_through("cap-fast");
    {
        const long fs = strtol(get("cap-fast").c_str(), nullptr, 10);   // (the whole number: CAP_FAST is its low 32 bits)
        const int threads = std::max(1, std::min(8, THREADS_PER_MCTS));
        if (CAP_PROB < 1.0f && fs > 0 && (fs < threads || fs > MCTS_SIMULATIONS)) {   // the cap is on: F - F % T descents, at most a full decision's
            fprintf(stderr, "--cap-fast: %ld simulations are outside [%d search threads (-t), %d simulations (--mcts)]\n", fs, threads, MCTS_SIMULATIONS);
            exit(2);
        }
    }
    fill_through("prune-target");
    if (PRUNE_TARGET == 1 && !(FORCED_K > 0.0f)) {
        fprintf(stderr, "--prune-target: 1 needs --forced-k above 0 (pruning subtracts forced playouts; there are none)\n");
        exit(2);
    }
    fill_through("gumbel-tree");   // (--gumbel-m with --dir-alpha is not refused here: azr_selfplay_start refuses it)
    if (GUMBEL_TREE == 1 && GUMBEL_M == 0) {
        fprintf(stderr, "--gumbel-tree: 1 needs --gumbel-m above 0 (the selection below the root belongs to the Gumbel root search)\n");
        exit(2);
    }
    fill_through("arena-gumbel-tree2");
    // player 2's search: player 1's unless given (the settings file then carries the value in force, as for --mcts2)
    if (!given.count("arena-gumbel-m2")) { ARENA_GUMBEL_M2 = ARENA_GUMBEL_M; val["arena-gumbel-m2"] = get("arena-gumbel-m"); }
    if (!given.count("arena-gumbel-tree2")) { ARENA_GUMBEL_TREE2 = ARENA_GUMBEL_TREE; val["arena-gumbel-tree2"] = get("arena-gumbel-tree"); }
    if (ARENA_GUMBEL_TREE == 1 && ARENA_GUMBEL_M == 0) {
        fprintf(stderr, "--arena-gumbel-tree: 1 needs --arena-gumbel-m above 0 (the selection below the root belongs to the Gumbel root search)\n");
        exit(2);
    }
    if (ARENA_GUMBEL_TREE2 == 1 && ARENA_GUMBEL_M2 == 0) {
        fprintf(stderr, "--arena-gumbel-tree2: 1 needs --arena-gumbel-m2 above 0 (the selection below the root belongs to the Gumbel root search)\n");
        exit(2);
    }
    fill_through("");
    for (auto& o : train_opts) fill(o);
    LR_SCHEDULE = get("lr-schedule");
    {   // what azr_nn_train_set_options would refuse, before an engine exists
        const bool cosine = LR_SCHEDULE == "cosine", step = LR_SCHEDULE == "step";
        if (!cosine && !step && LR_SCHEDULE != "constant") {
            fprintf(stderr, "--lr-schedule: unknown schedule '%s' (constant|cosine|step)\n", LR_SCHEDULE.c_str());
            exit(2);
        }
        if (cosine && LR_STEPS <= LR_WARMUP) {
            fprintf(stderr, "--lr-steps: %d steps do not lie behind the warm-up's %d (--lr-schedule cosine needs --lr-steps above --lr-warmup)\n", LR_STEPS, LR_WARMUP);
            exit(2);
        }
        if (cosine && LR_MIN > LR) {
            fprintf(stderr, "--lr-min: %g is not a floor of the cosine schedule (a number in [0, --lr %g])\n", LR_MIN, LR);
            exit(2);
        }
        if (EMA_PLAY == 1 && !(EMA_DECAY > 0.0f)) {
            fprintf(stderr, "--ema-play: 1 needs --ema-decay above 0 (there is no averaged net to play)\n");
            exit(2);
        }
    }
    CV_K = atoi(get("cvk").c_str());
    CV_MAX_EPOCHS = atoi(get("cv-max-epochs").c_str());
    DEVICE_MAP.clear();
    {
        std::stringstream ss(get("devices"));
        std::string tok;
        while (std::getline(ss, tok, ',')) if (!tok.empty()) DEVICE_MAP.push_back(atoi(tok.c_str()));
        if (!DEVICE_MAP.empty() && (int)DEVICE_MAP.size() != NUMBER_OF_GPUS) {
            fprintf(stderr, "--devices names %d devices for --gpus %d\n", (int)DEVICE_MAP.size(), NUMBER_OF_GPUS);
            exit(2);
        }
    }
    // `--lnt` and `--apbs` are parsed and never applied in the reference either
    mkdirs("log");
    std::ofstream out("log/settings.txt", std::ofstream::out);
    for (const std::vector<Opt>* t : {(const std::vector<Opt>*)&opts, &train_opts})
        for (auto& o : *t) out << o.name << "(" << o.desc << ")=" << (val.count(o.name) ? val[o.name] : o.def) << std::endl;
}

azr_train_options Settings::trainOptions() const
{
    azr_train_options o;
    azr_default_train_options(&o);
    o.lr = LR; o.l2 = L2;
    o.lr_schedule = LR_SCHEDULE == "cosine" ? AZR_LR_COSINE : LR_SCHEDULE == "step" ? AZR_LR_STEP : AZR_LR_CONSTANT;
    o.warmup_steps = LR_WARMUP; o.total_steps = LR_STEPS; o.lr_min = LR_MIN;
    o.decay_period = LR_PERIOD; o.decay_gamma = LR_GAMMA;
    o.clip_norm = CLIP_NORM; o.ema_decay = EMA_DECAY;
    return o;
}

bool Settings::trainOptionsDefault() const
{
    return LR == 1e-3f && L2 == 1e-3f && LR_SCHEDULE == "constant" && LR_WARMUP == 0 && CLIP_NORM == 0.0f && EMA_DECAY == 0.0f;
}

void Settings::toEngine(azr_settings& s, int device) const
{
    azr_default_settings(&s);
    s.device = device;
    s.games = NUMBER_OF_CONCURENT_GAMES_PER_GPU;
    s.blocks = BLOCKS;
    s.net_dtype = netDtype(NET_DTYPE);
    s.mcts_simulations = MCTS_SIMULATIONS;
    s.mcts_threads = std::max(1, std::min(8, THREADS_PER_MCTS));
    s.allow_yield = ALLOW_YIELD;
    s.limit_reinforcement = LIMIT_REINFORCEMENT_MOVES;
    s.limit_attack = LIMIT_ATTACK_MOVES;
    s.max_game_rounds = MAX_GAME_ROUNDS;
    s.min_unit_move = MIN_UNIT_MOVE;
    s.temperature_threshold = TEMPERATURE_TRESHOLD;
    s.hp_exploration = HP_EXPLORATION;
    s.dir_noise_value = DIR_NOISE_VALUE;
    s.dir_noise_epsi = DIR_NOISE_EPSI;
    // player 2's tree lives in a pool of the same size as player 1's: make room for the larger of the two budgets
    // (only where player 2 searches: -m play --p1 az --p2 az)
    if (MODE == "play" && PLAYER_1 == "az" && PLAYER_2 == "az" && MCTS_SIMULATIONS2 > MCTS_SIMULATIONS) s.node_capacity = 16 * (MCTS_SIMULATIONS2 + 1);
}

int Settings::netDtype(const std::string& name)
{
    return name == "f32" ? AZR_NET_F32 : name == "f32x" ? AZR_NET_F32X : name == "f16" ? AZR_NET_F16 : AZR_NET_BF16;
}

std::string Settings::describe() const
{
    std::ostringstream o;
    o << "GPUs: " << NUMBER_OF_GPUS << ", Games per GPU " << NUMBER_OF_CONCURENT_GAMES_PER_GPU << ", MCTS threads: "
      << THREADS_PER_MCTS << ", MCTS simulations " << MCTS_SIMULATIONS;
    return o.str();
}

// ---- samples ---------------------------------------------------------------------------------------------------------
void NNTrainDataStorage::appendPacked(const uint8_t* rec, size_t n)
{
    data.reserve(data.size() + n);
    for (size_t i = 0; i < n; i++, rec += AZR_RECORD_BYTES) {
        NNTrainData d;
        d.playerIndex = (int8_t)rec[0];
        memcpy(d.in.bytes, rec + 1, AZR_INPUT_BYTES);
        memcpy(&d.out.value, rec + 89, 4);
        d.out.policy.resize(AZR_MOVES);
        memcpy(d.out.policy.data(), rec + 93, AZR_MOVES * 4);
        data.push_back(std::move(d));
    }
}

void NNTrainDataStorage::trimOldExamples()
{
    if (data.size() > (size_t)SETTINGS.SAMPLES_STORAGE_MAX) {
        size_t excess = data.size() - SETTINGS.SAMPLES_STORAGE_MAX;
        data.erase(data.begin(), data.begin() + excess);
        printf("[MAX] Erased %d oldeset examples\n", int(excess));
    } else if (data.size() > (size_t)SETTINGS.SAMPLES_STORAGE_MIN && oldGameIndex > 0) {
        size_t excess = std::min(oldGameIndex, data.size() - SETTINGS.SAMPLES_STORAGE_MIN);
        oldGameIndex -= excess;
        data.erase(data.begin(), data.begin() + excess);
        printf("[MIN] Erased %d oldeset examples\n", int(excess));
    }
}

void NNTrainDataStorage::updateValues(int gameStatus, int roundCount)
{
    (void)roundCount;  // ROUND_WEIGHTED_VALUE is not a default macro
    for (size_t i = lastGameIndex; i < data.size(); i++)
        data[i].out.value = gameStatus == State::DRAW ? 0.0f : data[i].playerIndex == gameStatus ? 1.0f : -1.0f;
    lastGameIndex = data.size();
}

std::vector<uint8_t> NNTrainDataStorage::packed() const
{
    std::vector<uint8_t> buf(data.size() * AZR_RECORD_BYTES);
    for (size_t i = 0; i < data.size(); i++) {
        uint8_t* r = buf.data() + i * AZR_RECORD_BYTES;
        r[0] = (uint8_t)data[i].playerIndex;
        memcpy(r + 1, data[i].in.bytes, AZR_INPUT_BYTES);
        memcpy(r + 89, &data[i].out.value, 4);
        memcpy(r + 93, data[i].out.policy.data(), 4 * AZR_MOVES);
    }
    return buf;
}

void NNTrainDataStorage::saveTrainingSamples(const std::string& path) const
{
    if (data.empty()) { printf("No training samples\n"); return; }
    size_t slash = path.find_last_of('/');
    if (slash != std::string::npos) mkdirs(path.substr(0, slash));
    std::ofstream out(path, std::ios::out | std::ios::binary);
    uint64_t size = data.size();
    out.write((const char*)&size, 8);
    for (auto& d : data) {
        out.write((const char*)&d.playerIndex, 1);
        out.write((const char*)d.in.bytes, AZR_INPUT_BYTES);
        out.write((const char*)&d.out.value, 4);
        out.write((const char*)d.out.policy.data(), 4 * AZR_MOVES);
    }
    printf("Training samples saved %d\n", int(data.size()));
}

void NNTrainDataStorage::loadTrainingSamples(const std::string& path)
{
    std::ifstream in(path, std::ios::in | std::ios::binary | std::ios::ate);
    if (!in) { printf("File does note exist: %s\n", path.c_str()); return; }
    const uint64_t bytes = (uint64_t)in.tellg();
    in.seekg(0);
    // the reference's writer emits an 8-byte count, its reader consumes 4 bytes: accept whichever fits the file size
    uint64_t n8 = 0;
    in.read((char*)&n8, 8);
    size_t header = 8;
    uint64_t n = n8;
    if (bytes != 8 + n8 * AZR_RECORD_BYTES) {
        uint32_t n4 = (uint32_t)n8;
        if (bytes == 4 + (uint64_t)n4 * AZR_RECORD_BYTES) { n = n4; header = 4; }
        else { printf("Unrecognised sample file: %s\n", path.c_str()); return; }
    }
    in.seekg(header);
    std::vector<uint8_t> buf(n * AZR_RECORD_BYTES);
    in.read((char*)buf.data(), buf.size());
    appendPacked(buf.data(), n);
}

// ---- engine / NN service ------------------------------------------------------------------------------------------
Engine::Engine(const Settings& s, int device, int g) : games(g)
{
    azr_settings es;
    s.toEngine(es, device);
    es.games = g;
    int rc = azr_engine_create(&es, &h);
    if (rc) {
        std::string msg = azr_last_error(nullptr);   // *out is NULL on failure; the reason is kept per thread
        h = nullptr;
        throw std::runtime_error("engine: " + msg);
    }
    setTrainOptions(s);
}
// the optimiser step's options, once per engine: they stay on the handle
void Engine::setTrainOptions(const Settings& s)
{
    const azr_train_options o = s.trainOptions();
    check(azr_nn_train_set_options(h, &o), "train_set_options");
}
Engine::Engine(const Settings& s, int device, int g, int blocks, const std::string& dtype) : games(g)
{
    azr_settings es;
    s.toEngine(es, device);
    es.games = g;
    es.blocks = blocks;
    es.net_dtype = Settings::netDtype(dtype);
    int rc = azr_engine_create(&es, &h);
    if (rc) {
        std::string msg = azr_last_error(nullptr);
        h = nullptr;
        throw std::runtime_error("engine: " + msg);
    }
    setTrainOptions(s);
}
Engine::~Engine() { if (h) azr_engine_destroy(h); }
void Engine::check(int rc, const char* what) const
{
    if (rc == AZR_E_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + azr_last_error(h));
    if (rc == AZR_E_LOGIC) throw std::logic_error(std::string(what) + ": " + azr_last_error(h));
    if (rc) throw std::runtime_error(std::string(what) + ": " + azr_last_error(h));
}

void AlphaZeroNNId::loadCheckpoint(const std::string& path)
{
    struct stat st;
    rawWeights.clear();   // (the weights of a training phase are replaced: there is nothing to put back)
    if (stat(path.c_str(), &st) == 0) {
        engine->check(azr_nn_load(engine->h, path.c_str()), "loadCheckpoint");
        printf("Loaded checkpoint %s\n", path.c_str());
    } else {  // alphazero_nn.cpp:197-202: no checkpoint => initialise and save one
        printf("Checkpoint %s not found, initializing random weights\n", path.c_str());
        engine->check(azr_nn_init_random(engine->h, 20260002ull), "init");
        saveCheckpoint(path);
    }
}
void AlphaZeroNNId::saveCheckpoint(const std::string& path)
{
    size_t slash = path.find_last_of('/');
    if (slash != std::string::npos) mkdirs(path.substr(0, slash));
    engine->check(azr_nn_save(engine->h, path.c_str()), "saveCheckpoint");
}
NNOutputData AlphaZeroNNId::predict(const NNInputData& in) { return predict(std::vector<NNInputData>{in})[0]; }
std::vector<NNOutputData> AlphaZeroNNId::predict(const std::vector<NNInputData>& in)
{
    const int n = (int)in.size();
    std::vector<uint8_t> x((size_t)n * AZR_INPUT_BYTES);
    for (int i = 0; i < n; i++) memcpy(x.data() + (size_t)i * AZR_INPUT_BYTES, in[i].bytes, AZR_INPUT_BYTES);
    std::vector<float> pi((size_t)n * AZR_MOVES), v(n);
    engine->check(azr_nn_predict(engine->h, x.data(), n, pi.data(), v.data()), "predict");
    std::vector<NNOutputData> out(n);
    for (int i = 0; i < n; i++) {
        out[i].policy.assign(pi.begin() + (size_t)i * AZR_MOVES, pi.begin() + (size_t)(i + 1) * AZR_MOVES);
        out[i].value = v[i];
    }
    return out;
}

// stands in for the process-global RNG engine the reference shuffles with (src/rng.h:50); raw minstd_rand0 state
static uint32_t g_shuffle_state = 1;
static std::ofstream& logFile(const char* path)
{
    static std::map<std::string, std::ofstream> files;
    auto& f = files[path];
    if (!f.is_open()) { mkdirs("log"); f.open(path, std::ofstream::out | std::ofstream::app); }
    return f;
}

void AlphaZeroNNId::train(const std::vector<NNTrainData>& trainData, int epochs)
{
    std::vector<uint8_t> buf(trainData.size() * AZR_RECORD_BYTES);
    for (size_t i = 0; i < trainData.size(); i++) {
        uint8_t* r = buf.data() + i * AZR_RECORD_BYTES;
        r[0] = (uint8_t)trainData[i].playerIndex;
        memcpy(r + 1, trainData[i].in.bytes, AZR_INPUT_BYTES);
        memcpy(r + 89, &trainData[i].out.value, 4);
        memcpy(r + 93, trainData[i].out.policy.data(), 4 * AZR_MOVES);
    }
    printf("Started training\n");
    trainRaw();
    std::vector<float> lp(std::max(epochs, 1)), lv(std::max(epochs, 1));
    auto t0 = std::chrono::steady_clock::now();
    engine->check(azr_nn_train(engine->h, buf.data(), trainData.size(), epochs, SETTINGS.BATCH_SIZE, &g_shuffle_state, lp.data(), lv.data()),
                  "train");
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int e = 0; e < epochs; e++) {
        printf("EPOCH %d\nLoss Policy / Value: %f / %f\n", e, lp[e], lv[e]);
        if (SETTINGS.LOG_NN_TRAINING) logFile("log/azr-nn-training-log.txt") << lp[e] << ", " << lv[e] << ", ";
    }
    if (SETTINGS.LOG_NN_TRAINING) logFile("log/azr-nn-training-log.txt") << std::endl;
    const size_t steps = (size_t)epochs * (trainData.size() / SETTINGS.BATCH_SIZE);
    printf("Trained %zu minibatch steps of %d in %.2f s (%.1f ms/step)\n", steps, SETTINGS.BATCH_SIZE, dt, steps ? 1e3 * dt / steps : 0.0);
    if (steps) { logOptimiser(steps); playAveraged(); }
}

void AlphaZeroNNId::logOptimiser(size_t steps)
{
    if (SETTINGS.trainOptionsDefault()) return;
    azr_train_stats st;
    engine->check(azr_nn_train_stats(engine->h, &st), "train_stats");
    char norm[32] = "n/a";
    if (!std::isnan(st.grad_norm)) snprintf(norm, sizeof norm, "%.6g", st.grad_norm);
    printf("Optimiser step: lr %.6g, grad norm %s, clipped %lld/%lld steps   [%zu steps in this phase]%s\n", st.lr, norm, (long long)st.clipped_steps,
           (long long)st.step, steps, SETTINGS.EMA_PLAY ? "   [the averaged net plays]" : "");
}

// --ema-play 1, behind a training phase: keep the raw weights, hold the averaged ones (azr_nn_set_weights keeps the training context)
void AlphaZeroNNId::playAveraged()
{
    if (!SETTINGS.EMA_PLAY) return;
    const size_t n = azr_nn_param_count(SETTINGS.BLOCKS);
    rawWeights.resize(n);
    std::vector<float> ema(n);
    engine->check(azr_nn_get_weights(engine->h, rawWeights.data(), n), "get_weights");
    engine->check(azr_nn_get_ema_weights(engine->h, ema.data(), n), "get_ema_weights");
    engine->check(azr_nn_set_weights(engine->h, ema.data(), n), "set_weights");
}
// ... and in front of the next one: training goes on with the raw weights
void AlphaZeroNNId::trainRaw()
{
    if (rawWeights.empty()) return;
    engine->check(azr_nn_set_weights(engine->h, rawWeights.data(), rawWeights.size()), "set_weights");
    rawWeights.clear();
}

// ---- cross-validation (`-m analysis`) ---------------------------------------------------------------------------------
static uint32_t engineState(const std::minstd_rand0& eng)   // minstd_rand0 has no state accessor; operator<< prints it
{
    std::ostringstream os;
    os << eng;
    return (uint32_t)std::stoul(os.str());
}
static std::vector<uint8_t> packRecords(const std::vector<const NNTrainData*>& v)
{
    std::vector<uint8_t> buf(v.size() * AZR_RECORD_BYTES);
    for (size_t i = 0; i < v.size(); i++) {
        uint8_t* r = buf.data() + i * AZR_RECORD_BYTES;
        r[0] = (uint8_t)v[i]->playerIndex;
        memcpy(r + 1, v[i]->in.bytes, AZR_INPUT_BYTES);
        memcpy(r + 89, &v[i]->out.value, 4);
        memcpy(r + 93, v[i]->out.policy.data(), 4 * AZR_MOVES);
    }
    return buf;
}

// The reference takes its `lock` (a plain std::mutex) here and then calls initWeights() / saveCheckpoint(), which take it again: as
// written it deadlocks in the first fold.  This is what it evidently intends, without the lock.  Every draw of the
// global RNG — the fold shuffle, then per epoch the training-set and the validation-set shuffle — comes from g_shuffle_state, as for
// `train`.  A fold starts from azr_nn_init_random(20260002 + vi) with the optimiser state dropped (TF's init op resets the Adam slots).
void AlphaZeroNNId::trainCrossValidation(const std::vector<NNTrainData>& trainData, int k)
{
    if (k < 1) throw std::invalid_argument("trainCrossValidation: need k >= 1 folds");
    std::vector<const NNTrainData*> shuffleTrainData(trainData.size());
    for (size_t i = 0; i < trainData.size(); i++) shuffleTrainData[i] = &trainData[i];
    const int crossValidationGroupSize = (int)(shuffleTrainData.size() / k);
    float previousBestEpochLossV = 0.0f;
    std::minstd_rand0 eng;
    printf("Started cross-validation training\n");
    for (int vi = 0; vi < k; vi++) {
        printf("Cross-validation step: %d/%d\n", vi, k);
        engine->check(azr_nn_init_random(engine->h, 20260002ull + (uint64_t)vi), "initWeights");
        engine->check(azr_nn_train_reset(engine->h), "initWeights");
        if (vi % k == 0) {
            eng.seed(g_shuffle_state);
            std::shuffle(shuffleTrainData.begin(), shuffleTrainData.end(), eng);
            g_shuffle_state = engineState(eng);
        }
        std::vector<const NNTrainData*> trainingSamples, validationSamples;
        const int start = vi * crossValidationGroupSize, end = (vi + 1) * crossValidationGroupSize;   // (index `start` trains)
        for (int i = 0; i < (int)shuffleTrainData.size(); i++) (start < i && i < end ? validationSamples : trainingSamples).push_back(shuffleTrainData[i]);

        bool modelLearning = true;
        int failedImprovement = 0;
        for (int e = 0; (e < SETTINGS.EPOCHS || modelLearning) && (SETTINGS.CV_MAX_EPOCHS <= 0 || e < SETTINGS.CV_MAX_EPOCHS); e++) {
            printf("EPOCH %d\n", e);
            {   // training phase: azr_nn_train shuffles the records it is given with the same engine and state, i.e. it trains on the
                // minibatches of the shuffled trainingSamples; the host vector takes the same permutation
                const std::vector<uint8_t> buf = packRecords(trainingSamples);
                uint32_t st = g_shuffle_state;
                float lp = NAN, lv = NAN;
                engine->check(azr_nn_train(engine->h, buf.data(), trainingSamples.size(), 1, SETTINGS.BATCH_SIZE, &st, &lp, &lv), "train");
                eng.seed(g_shuffle_state);
                std::shuffle(trainingSamples.begin(), trainingSamples.end(), eng);
                if (engineState(eng) != st) throw std::logic_error("trainCrossValidation: host and device shuffle streams diverged");
                std::shuffle(validationSamples.begin(), validationSamples.end(), eng);
                g_shuffle_state = engineState(eng);
                printf("Training Loss Policy %f Value: %f\n", lp, lv);
                if (trainingSamples.size() >= (size_t)SETTINGS.BATCH_SIZE) logOptimiser(trainingSamples.size() / SETTINGS.BATCH_SIZE);
                saveCheckpoint(SETTINGS.DEFAULT_CHECKPOINT_DIR + "/cross-validation-" + std::to_string(vi) + "-" + std::to_string(e) + " .bin");
                logFile("log/azr-nn-training-log.txt") << lp << "," << lv;
            }
            {   // validation phase: the same loss with batch norm on the moving statistics, no update
                const std::vector<uint8_t> buf = packRecords(validationSamples);
                float vlp = NAN, vlv = NAN;
                engine->check(azr_nn_validate(engine->h, buf.data(), validationSamples.size(), SETTINGS.BATCH_SIZE, &vlp, &vlv, nullptr, nullptr),
                              "validate");
                printf("Validation Loss Policy %f Value: %f\n", vlp, vlv);
                logFile("log/azr-nn-training-log.txt") << "," << vlp << "," << vlv << std::endl;
                if (e == 0) {
                    previousBestEpochLossV = vlv;
                } else {
                    const float diffAvgLoss = previousBestEpochLossV - vlv;
                    if (diffAvgLoss > 0 && diffAvgLoss > previousBestEpochLossV * SETTINGS.DYNAMIC_EPOCH_THRESHOLD) {   // improved on validation
                        previousBestEpochLossV = vlv;
                        failedImprovement = 0;
                    } else if (++failedImprovement == 3) {
                        printf("=> Stopped training model is not learning\n");
                        modelLearning = false;
                    }
                }
            }
        }
    }
}

void AlphaZeroNNGroup::train(const std::vector<NNTrainData>& trainData, int epochs)
{
    auto& nn = neuralNetworkIds.at(0);
    nn->train(trainData, epochs);
    nn->saveCheckpoint(SETTINGS.DEFAULT_CHECKPOINT_TEMP);
    for (size_t i = 1; i < neuralNetworkIds.size(); i++) neuralNetworkIds[i]->loadCheckpoint(SETTINGS.DEFAULT_CHECKPOINT_TEMP);
}

std::shared_ptr<AlphaZeroNNGroup> AlphaZeroCluster::initPlayerGroup(const std::string& name, const std::string& graphPath, int blocks, const std::string& dtype)
{
    for (auto& g : groups)
        if (g->name == name) throw std::invalid_argument("Duplicated player group");  // alphazero_gpu_cluster.cpp:160-163
    (void)graphPath;  // the TF graph-def is not used: the net is built into the HIP library, its shape is `blocks` / `dtype`
    auto grp = std::make_shared<AlphaZeroNNGroup>();
    grp->name = name;
    for (int gpu = 0; gpu < gpus; gpu++) {
        auto eng = std::make_shared<Engine>(SETTINGS, SETTINGS.deviceOf(gpu), SETTINGS.NUMBER_OF_CONCURENT_GAMES_PER_GPU, blocks, dtype);
        grp->neuralNetworkIds.push_back(std::make_shared<AlphaZeroNNId>(eng, gpu));
    }
    groups.push_back(grp);
    return grp;
}

// ---- search ------------------------------------------------------------------------------------------------------------
void AlphaZeroMCTS::clearNodes() { nn->engine->check(azr_mcts_clear(nn->engine->h), "clearNodes"); }
void AlphaZeroMCTS::trimNodes() { nn->engine->check(azr_mcts_trim(nn->engine->h), "trimNodes"); }
void AlphaZeroMCTS::simulate(const std::vector<State>& roots)
{
    Engine& e = *nn->engine;
    if ((int)roots.size() != e.games) throw std::invalid_argument("simulate: one root per engine game expected");
    std::vector<uint8_t> img((size_t)e.games * AZR_STATE_BYTES);
    for (int g = 0; g < e.games; g++) memcpy(img.data() + (size_t)g * AZR_STATE_BYTES, roots[g].data, AZR_STATE_BYTES);
    e.check(azr_engine_set_states(e.h, img.data()), "set_states");
    e.check(azr_mcts_simulate(e.h), "simulate");
}
std::vector<std::vector<float>> AlphaZeroMCTS::calculateMoveProbability()
{
    Engine& e = *nn->engine;
    std::vector<float> pi((size_t)e.games * AZR_MOVES);
    e.check(azr_mcts_policy(e.h, pi.data()), "policy");
    std::vector<std::vector<float>> out(e.games);
    for (int g = 0; g < e.games; g++) out[g].assign(pi.begin() + (size_t)g * AZR_MOVES, pi.begin() + (size_t)(g + 1) * AZR_MOVES);
    return out;
}
std::vector<uint8_t> AlphaZeroMCTS::pickHigestWeightedMove()
{
    std::vector<uint8_t> mv(nn->engine->games);
    nn->engine->check(azr_mcts_pick(nn->engine->h, 0, mv.data()), "pick");
    return mv;
}
std::vector<uint8_t> AlphaZeroMCTS::pickRandomWeightedMove()
{
    std::vector<uint8_t> mv(nn->engine->games);
    nn->engine->check(azr_mcts_pick(nn->engine->h, 1, mv.data()), "pick");
    return mv;
}

AlphaZeroPlayerGroup::AlphaZeroPlayerGroup(std::shared_ptr<AlphaZeroNNGroup> g) : nnGroup(g)
{
    for (size_t i = 0; i < g->size(); i++)
        for (int k = 0; k < SETTINGS.NUMBER_OF_CONCURENT_GAMES_PER_GPU; k++) players.push_back(std::make_shared<Player>());
}

void AlphaZeroPlayerGroup::takeTurns(int gpu, std::vector<State>& states, int8_t playerIndexTurn, std::vector<NNTrainDataStorage>* storages)
{
    auto nn = nnGroup->getNN(gpu);
    Engine& e = *nn->engine;
    AlphaZeroMCTS mcts(nn);
    const int G = e.games;
    if ((int)states.size() != G) throw std::invalid_argument("takeTurns: one State per engine game expected");
    std::vector<uint8_t> img((size_t)G * AZR_STATE_BYTES);
    std::vector<int8_t> status(G);
    mcts.trimNodes();  // AlphaZeroPlayer::takeTurn's own trim (alphazero_player.cpp:5)
    for (;;) {
        for (int g = 0; g < G; g++) memcpy(img.data() + (size_t)g * AZR_STATE_BYTES, states[g].data, AZR_STATE_BYTES);
        e.check(azr_engine_set_states(e.h, img.data()), "set_states");
        e.check(azr_engine_status(e.h, status.data()), "status");
        bool any = false;
        for (int g = 0; g < G; g++) any |= status[g] == -1 && states[g].getCurrentPlayerTurn() == playerIndexTurn;
        if (!any) break;
        e.check(azr_mcts_simulate(e.h), "simulate");
        std::vector<uint8_t> mv = mcts.pickHigestWeightedMove();
        for (int g = 0; g < G; g++)
            if (!(status[g] == -1 && states[g].getCurrentPlayerTurn() == playerIndexTurn)) mv[g] = 255;
        if (storages) {  // alphazero_player.cpp:15-18
            std::vector<uint8_t> in88((size_t)G * AZR_INPUT_BYTES);
            std::vector<float> pi((size_t)G * AZR_MOVES);
            e.check(azr_engine_encode(e.h, in88.data()), "encode");
            e.check(azr_mcts_policy(e.h, pi.data()), "policy");
            for (int g = 0; g < G; g++) {
                if (mv[g] == 255) continue;
                NNTrainData d;
                d.playerIndex = playerIndexTurn;
                memcpy(d.in.bytes, in88.data() + (size_t)g * AZR_INPUT_BYTES, AZR_INPUT_BYTES);
                d.out.policy.assign(pi.begin() + (size_t)g * AZR_MOVES, pi.begin() + (size_t)(g + 1) * AZR_MOVES);
                (*storages)[g].data.push_back(std::move(d));
            }
        }
        e.check(azr_engine_make_moves(e.h, mv.data(), nullptr), "makeMove");
        e.check(azr_engine_get_states(e.h, img.data()), "get_states");
        for (int g = 0; g < G; g++) memcpy(states[g].data, img.data() + (size_t)g * AZR_STATE_BYTES, AZR_STATE_BYTES);
    }
}

// ---- trainer ------------------------------------------------------------------------------------------------------------
// the self-play options of the command line (--help says what each does), in force for the games generated from here on
static void applySelfplayOptions(Engine& e)
{
    const Settings& s = SETTINGS;
    e.check(azr_selfplay_set_dirichlet(e.h, s.DIR_ALPHA, s.DIR_SEED), "selfplay_set_dirichlet");
    e.check(azr_selfplay_set_playout_cap(e.h, s.CAP_PROB, s.CAP_FAST, s.CAP_SEED), "selfplay_set_playout_cap");
    e.check(azr_selfplay_set_forced_playouts(e.h, s.FORCED_K, s.PRUNE_TARGET), "selfplay_set_forced_playouts");
    e.check(azr_selfplay_set_surprise_weighting(e.h, s.PSW_SHARE, s.PSW_MAX, s.PSW_SEED), "selfplay_set_surprise_weighting");
    e.check(azr_selfplay_set_value_mix(e.h, s.Q_SHARE), "selfplay_set_value_mix");
    e.check(azr_selfplay_set_resign(e.h, s.RESIGN_Q, s.RESIGN_STREAK, s.RESIGN_HOLDOUT, s.RESIGN_SEED), "selfplay_set_resign");
    e.check(azr_selfplay_set_gumbel(e.h, s.GUMBEL_M, s.GUMBEL_CVISIT, s.GUMBEL_CSCALE, s.GUMBEL_SEED), "selfplay_set_gumbel");
    e.check(azr_selfplay_set_gumbel_tree(e.h, s.GUMBEL_TREE), "selfplay_set_gumbel_tree");
}

SelfPlayReport AlphaZeroTrainer::generateTrainData(std::shared_ptr<AlphaZeroNNGroup> generate)
{
    const int P = (int)generate->size();
    const uint64_t target = (uint64_t)SETTINGS.TRAIN_ITERATION_GAMES;
    printf("Generating training data current sample count %d\n", int(trainStorage.data.size()));
    std::vector<NNTrainDataStorage> storageGroup(P);
    std::vector<SelfPlayReport> rep(P);
    // GPU i's seed stream: base + i * 2^24 + (games this GPU has started in earlier iterations) — no game of any
    // (iteration, GPU) pair is ever replayed.  Shares, seeds and the stream positions are fixed HERE, by the parent, before
    // any thread exists: the threads only read their own copies.
    if (selfPlayStarted.size() < (size_t)P) selfPlayStarted.resize(P, 0);
    std::vector<uint64_t> shares(P);
    std::vector<uint32_t> seeds(P);
    for (int i = 0; i < P; i++) {
        shares[i] = target / P + ((uint64_t)i < target % P ? 1 : 0);
        seeds[i] = SETTINGS.BASE_SEED + (uint32_t)i * (1u << 24) + (uint32_t)selfPlayStarted[i];
        selfPlayStarted[i] += shares[i];
    }
    auto t0 = std::chrono::steady_clock::now();
    forEachGpu(P, "self-play", [&](int i) {  // one self-play thread per GPU (alphazero_trainer.cpp:48-57)
        const uint64_t share = shares[i];
        const uint32_t seed = seeds[i];
        if (share == 0) return;
        Engine& e = *generate->getNN(i)->engine;
        // exactly `share` games are started and every one is played to its end (Counter::hasNext over
        // TRAIN_ITERATION_GAMES, alphazero_trainer.cpp:83)
        applySelfplayOptions(e);
        e.check(azr_selfplay_start_games(e.h, seed, share), "selfplay_start_games");
        azr_counters c{};
        std::vector<uint8_t> buf((size_t)e.games * 512 * AZR_RECORD_BYTES);
        while (c.games_finished + c.errors < share) {
            e.check(azr_selfplay_run(e.h, 4 * (SETTINGS.MCTS_SIMULATIONS + 2)), "selfplay_run");
            e.check(azr_selfplay_counters(e.h, &c), "counters");
            if (c.records_dropped) throw std::runtime_error("self-play records were dropped (sample_capacity too small)");
            for (size_t n = buf.size() / AZR_RECORD_BYTES; n == buf.size() / AZR_RECORD_BYTES;) {  // a partial drain keeps the rest
                e.check(azr_samples_drain(e.h, buf.data(), buf.size() / AZR_RECORD_BYTES, &n), "drain");
                storageGroup[i].appendPacked(buf.data(), n);
            }
            printf("\r[gpu %d] games %llu/%llu  decisions %llu  simulations %llu", i, (unsigned long long)c.games_finished,
                   (unsigned long long)share, (unsigned long long)c.decisions, (unsigned long long)c.simulations);
            fflush(stdout);
        }
        rep[i].games = c.games_finished; rep[i].decisions = c.decisions; rep[i].simulations = c.simulations;
        rep[i].samples = storageGroup[i].data.size(); rep[i].errors = c.errors;
        e.check(azr_selfplay_resign_stats(e.h, &rep[i].resign), "resign_stats");
    });
    SelfPlayReport tot;
    tot.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t before = trainStorage.data.size();
    for (int i = 0; i < P; i++) {  // the "all-gather": concatenation in GPU order (alphazero_trainer.cpp:59-62)
        trainStorage.extend(storageGroup[i]);
        tot.games += rep[i].games; tot.decisions += rep[i].decisions; tot.simulations += rep[i].simulations;
        tot.samples += rep[i].samples; tot.errors += rep[i].errors;
        tot.resign.resigned += rep[i].resign.resigned; tot.resign.holdout_games += rep[i].resign.holdout_games;
        tot.resign.holdout_would_resign += rep[i].resign.holdout_would_resign; tot.resign.holdout_not_lost += rep[i].resign.holdout_not_lost;
    }
    printf("\nGenerated %d new samples for total %d\n", int(trainStorage.data.size() - before), int(trainStorage.data.size()));
    return tot;
}

void AlphaZeroTrainer::train(std::shared_ptr<AlphaZeroNNGroup> trainGroup, std::shared_ptr<AlphaZeroNNGroup> generateGroup)
{
    trainStorage.loadTrainingSamples(SETTINGS.DEFAULT_SAMPLES);
    printf("Started training\n");
    for (trainIteration = 0; trainIteration < SETTINGS.TRAIN_ITERATIONS; trainIteration++) {
        printf("Train iteration %ld\n", trainIteration);
        SelfPlayReport r = generateTrainData(generateGroup);
        printf("Self-play: %llu games, %llu decisions, %llu simulations in %.2f s  =>  %.0f simulations/s, %.2f games/s\n",
               (unsigned long long)r.games, (unsigned long long)r.decisions, (unsigned long long)r.simulations, r.seconds,
               r.simulations / r.seconds, r.games / r.seconds);
        if (SETTINGS.GUMBEL_M > 0)
            printf("Gumbel root search: m %d, c_visit %g, c_scale %g, seed %u%s\n", SETTINGS.GUMBEL_M, SETTINGS.GUMBEL_CVISIT, SETTINGS.GUMBEL_CSCALE,
                   SETTINGS.GUMBEL_SEED, SETTINGS.GUMBEL_TREE ? ", improved-policy selection below the root" : "");
        if (SETTINGS.RESIGN_STREAK > 0) {  // the holdout's false positives: would-be resigners that went on not to lose
            const azr_resign_stats& s = r.resign;
            printf("Resignation: %llu resigned, %llu held out, %llu of them would have resigned, %llu of those did not lose  =>  false-positive share ",
                   (unsigned long long)s.resigned, (unsigned long long)s.holdout_games, (unsigned long long)s.holdout_would_resign,
                   (unsigned long long)s.holdout_not_lost);
            if (s.holdout_would_resign) printf("%.3f\n", (double)s.holdout_not_lost / (double)s.holdout_would_resign);
            else printf("n/a\n");
        }
        trainStorage.trimOldExamples();
        trainGroup->train(trainStorage.data, SETTINGS.EPOCHS);
        if (updateIfImprovement(trainGroup, generateGroup, true)) trainStorage.updateOldGamesIndex();
    }
    trainStorage.saveTrainingSamples(SETTINGS.DEFAULT_SAMPLES);
}

// ---- game driver -----------------------------------------------------------------------------------------------------
void GameResults::add(const GameResults& o)
{
    count += o.count; draw += o.draw;
    for (int p = 0; p < 2; p++) { players[p].win += o.players[p].win; players[p].winAndStartedGame += o.players[p].winAndStartedGame; }
}
void GameResults::addGame(int gameStatus, int startingPlayer)  // game.cpp:193-213
{
    count++;
    if (gameStatus == State::DRAW) { draw++; return; }
    players[gameStatus].win++;
    if (gameStatus == startingPlayer) players[gameStatus].winAndStartedGame++;
}
std::ostream& operator<<(std::ostream& os, const GameResults& gr)  // game.cpp:227-235
{
    return os << gr.draw << ", " << gr.players[0].win << "/" << gr.players[0].winAndStartedGame << ", " << gr.players[1].win << "/"
              << gr.players[1].winAndStartedGame;
}

// every playGames call of a run plays other games: the reference draws from its process-global RNG, here a call counter
// moves the base seed (a compare / benchmark round must not replay the previous iteration's deals)
static std::atomic<uint32_t> arenaCallCounter{0};

// the first arena of the run with a Gumbel side says so once
static std::atomic<bool> arenaSearchLogged{false};

void GameGroup::applyArenaSearch(Engine& e, bool two, bool scripted)
{
    const Settings& s = SETTINGS;
    const int m1 = scripted ? 0 : s.ARENA_GUMBEL_M, m2 = two ? s.ARENA_GUMBEL_M2 : 0;
    e.check(azr_arena_set_gumbel(e.h, AZR_PLAYER_ALPHAZERO, m1, s.GUMBEL_CVISIT, s.GUMBEL_CSCALE, m1 ? s.ARENA_GUMBEL_TREE : 0), "arena_set_gumbel");
    if (two) e.check(azr_arena_set_gumbel(e.h, AZR_PLAYER_ALPHAZERO_B, m2, s.GUMBEL_CVISIT, s.GUMBEL_CSCALE, m2 ? s.ARENA_GUMBEL_TREE2 : 0), "arena_set_gumbel");
    if ((m1 > 0 || m2 > 0) && !arenaSearchLogged.exchange(true)) {
        auto side = [](int m, int tree) { return m > 0 ? "Gumbel m " + std::to_string(m) + (tree ? " (tree)" : "") : std::string("PUCT"); };
        if (two) printf("Arena search: player 1 %s, player 2 %s\n", side(m1, s.ARENA_GUMBEL_TREE).c_str(), side(m2, s.ARENA_GUMBEL_TREE2).c_str());
        else printf("Arena search: player 1 %s\n", side(m1, s.ARENA_GUMBEL_TREE).c_str());
    }
}

GameResults GameGroup::playGames(AlphaZeroPlayerGroup& pg1, AlphaZeroPlayerGroup& pg2, int games, NNTrainDataStorage* tds, int mcts2, float hp2)
{
    const uint32_t arenaCallsBase = ++arenaCallCounter;
    // Device-resident arena: pg1's engine of GPU i runs the G slots, pg2's network of the same GPU plays
    // AZR_PLAYER_ALPHAZERO_B (own tree per slot, evaluated on its own leaves).  Every slot is one of the reference's
    // threadPlayGame threads taking mirrored pairs from the shared counter (game.cpp:238-254).
    const int P = (int)pg1.nnGroup->size();
    printf("Playing games %d\n", games);
    std::vector<azr_game_results> res(P);
    std::vector<NNTrainDataStorage> st(P);
    const int pairs = games / 2;  // Counter::hasNext(2): whole pairs only
    const int mirror = SETTINGS.arenaMirrorMode();
    forEachGpu(P, "compare games", [&](int i) {
        Engine& e = *pg1.nnGroup->getNN(i)->engine;
        Engine& o = *pg2.nnGroup->getNN(i)->engine;
        memset(&res[i], 0, sizeof res[i]);
        const int share = 2 * (pairs / P + (i < pairs % P ? 1 : 0));
        if (share == 0) return;
        e.check(azr_arena_set_opponent_net(e.h, o.h), "arena_set_opponent_net");
        if (mcts2 >= 0 || hp2 >= 0) e.check(azr_arena_set_opponent_search(e.h, mcts2, hp2), "arena_set_opponent_search");
        applyArenaSearch(e, true);
        e.check(azr_arena_collect_samples(e.h, tds ? 1 : 0), "arena_collect_samples");
        const int passes = 4 * (std::max(SETTINGS.MCTS_SIMULATIONS, mcts2) + 2);   // the larger of the two budgets
        e.check(azr_arena_start(e.h, AZR_PLAYER_ALPHAZERO, AZR_PLAYER_ALPHAZERO_B, share, 0, mirror,
                                SETTINGS.BASE_SEED + 7919u * arenaCallsBase + (uint32_t)i * (1u << 24)), "arena_start");
        int fin = 0;
        std::vector<uint8_t> buf;
        while (!fin) {
            e.check(azr_arena_run(e.h, passes, &fin), "arena_run");
            e.check(azr_arena_results(e.h, &res[i]), "arena_results");
            if (tds) {
                buf.resize((size_t)e.games * 512 * AZR_RECORD_BYTES);
                for (size_t n = buf.size() / AZR_RECORD_BYTES; n == buf.size() / AZR_RECORD_BYTES;) {
                    e.check(azr_samples_drain(e.h, buf.data(), buf.size() / AZR_RECORD_BYTES, &n), "drain");
                    st[i].appendPacked(buf.data(), n);
                }
            }
            if (i == 0) {
                printf("\r%d/%d [Draw/P1,P2]: %d, %d/%d, %d/%d", res[i].count, share, res[i].draw, res[i].win[0], res[i].win_and_started[0],
                       res[i].win[1], res[i].win_and_started[1]);
                fflush(stdout);
            }
        }
        e.check(azr_arena_collect_samples(e.h, 0), "arena_collect_samples");
        e.check(azr_arena_set_opponent_net(e.h, nullptr), "arena_set_opponent_net");
    });
    printf("\n");
    GameResults all;
    for (auto& r : res) {
        all.count += r.count; all.draw += r.draw;
        for (int p = 0; p < 2; p++) { all.players[p].win += r.win[p]; all.players[p].winAndStartedGame += r.win_and_started[p]; }
    }
    if (tds) for (auto& s : st) tds->extend(s);
    return all;
}

// the arena's records so far, all of them, appended to `st` (the scripted-collection contract: drain after every run)
static void drainAll(Engine& e, NNTrainDataStorage& st)
{
    std::vector<uint8_t> buf((size_t)65536 * AZR_RECORD_BYTES);
    for (size_t n = 65536; n == 65536;) {
        e.check(azr_samples_drain(e.h, buf.data(), 65536, &n), "drain");
        st.appendPacked(buf.data(), n);
    }
}

// CONCURRENT pairs need two slots (azr_arena_start): an engine with one slot plays them one after the other
static int scriptedMirrorMode(const Engine& e)
{
    const int m = SETTINGS.arenaMirrorMode();
    return m == AZR_MIRROR_CONCURRENT && e.games < 2 ? AZR_MIRROR_SEQUENTIAL : m;
}

GameResults GameGroup::playGames(AlphaZeroPlayerGroup& pg1, int otherKind, int games, NNTrainDataStorage* tds)
{
    const uint32_t arenaCallsBase = ++arenaCallCounter;
    const int P = (int)pg1.nnGroup->size();
    printf("Playing games %d\n", games);
    std::vector<azr_game_results> res(P);
    std::vector<NNTrainDataStorage> st(P);
    const int pairs = games / 2;
    forEachGpu(P, "benchmark games", [&](int i) {
        Engine& e = *pg1.nnGroup->getNN(i)->engine;
        const int share = 2 * (pairs / P + (i < pairs % P ? 1 : 0));
        memset(&res[i], 0, sizeof res[i]);
        if (share == 0) return;
        const int mirror = tds ? scriptedMirrorMode(e) : SETTINGS.arenaMirrorMode();
        e.check(azr_arena_collect_samples(e.h, tds ? 1 : 0), "arena_collect_samples");
        e.check(azr_arena_collect_scripted_samples(e.h, tds ? 1 : 0), "arena_collect_scripted_samples");
        applyArenaSearch(e, false, tds != nullptr);
        e.check(azr_arena_start(e.h, AZR_PLAYER_ALPHAZERO, otherKind, share, 0, mirror,
                                SETTINGS.BASE_SEED + 104729u * arenaCallsBase + (uint32_t)i * (1u << 24)), "arena_start");
        int fin = 0;
        while (!fin) {
            e.check(azr_arena_run(e.h, 4 * (SETTINGS.MCTS_SIMULATIONS + 2), &fin), "arena_run");
            if (tds) drainAll(e, st[i]);
        }
        e.check(azr_arena_results(e.h, &res[i]), "arena_results");
        e.check(azr_arena_collect_samples(e.h, 0), "arena_collect_samples");
        e.check(azr_arena_collect_scripted_samples(e.h, 0), "arena_collect_scripted_samples");
    });
    if (tds) for (auto& s : st) tds->extend(s);
    GameResults all;
    for (auto& r : res) {
        all.count += r.count; all.draw += r.draw;
        for (int p = 0; p < 2; p++) { all.players[p].win += r.win[p]; all.players[p].winAndStartedGame += r.win_and_started[p]; }
    }
    return all;
}

int GameGroup::playScripted(AlphaZeroNNGroup& group, int kind0, int kind1, int games, NNTrainDataStorage& tds)
{
    const uint32_t arenaCallsBase = ++arenaCallCounter;
    const int P = (int)group.size();
    const int pairs = (games + 1) / 2;   // the arena plays whole mirrored pairs
    std::vector<NNTrainDataStorage> st(P);
    std::vector<int> played(P, 0);
    forEachGpu(P, "scripted games", [&](int i) {
        Engine& e = *group.getNN(i)->engine;
        const int share = 2 * (pairs / P + (i < pairs % P ? 1 : 0));
        if (share == 0) return;
        e.check(azr_arena_collect_samples(e.h, 0), "arena_collect_samples");
        e.check(azr_arena_collect_scripted_samples(e.h, 1), "arena_collect_scripted_samples");
        e.check(azr_arena_start(e.h, kind0, kind1, share, 0, scriptedMirrorMode(e),
                                SETTINGS.BASE_SEED + 15485863u * arenaCallsBase + (uint32_t)i * (1u << 24)), "arena_start");
        int fin = 0;
        while (!fin) {   // no network: one pass plays every slot's games to the end, or until the ring waits for a drain
            e.check(azr_arena_run(e.h, 2, &fin), "arena_run");
            drainAll(e, st[i]);
        }
        azr_game_results r{};
        e.check(azr_arena_results(e.h, &r), "arena_results");
        played[i] = r.count;
        e.check(azr_arena_collect_scripted_samples(e.h, 0), "arena_collect_scripted_samples");
    });
    int n = 0;
    for (int i = 0; i < P; i++) { tds.extend(st[i]); n += played[i]; }
    return n;
}

// ---- trainer: model selection (alphazero_trainer.cpp:121-198) ----------------------------------------------------------
void AlphaZeroTrainer::benchmark(AlphaZeroPlayerGroup& azpg)
{
    printf("Playing benchmark games with random\n");
    GameResults rGR = GameGroup::playGames(azpg, AZR_PLAYER_RANDOM, SETTINGS.BENCHMARK_GAMES_RANDOM);
    printf("Model benchmark games played: %d \t Model: %d/%d \t Random: %d/%d\n", rGR.count, rGR.players[0].win,
           rGR.players[0].winAndStartedGame, rGR.players[1].win, rGR.players[1].winAndStartedGame);
    printf("Playing benchmark games with script\n");
    GameResults sGR = GameGroup::playGames(azpg, AZR_PLAYER_SCRIPT, SETTINGS.BENCHMARK_GAMES_SCRIPT);
    printf("Model benchmark games played: %d \t Model: %d/%d \t Script: %d/%d\n", sGR.count, sGR.players[0].win,
           sGR.players[0].winAndStartedGame, sGR.players[1].win, sGR.players[1].winAndStartedGame);
    logFile("log/azr-benchmark-log.txt") << trainIteration << ',' << rGR << ", " << sGR << std::endl;
}

bool AlphaZeroTrainer::isModelImproved(const GameResults& gr)
{
    // int >= int * float: evaluated in float like the reference's expression (alphazero_trainer.cpp:197)
    return (float)gr.players[0].win >= (float)(gr.players[0].win + gr.players[1].win) * SETTINGS.COMPARE_TRESHOLD;
}

bool AlphaZeroTrainer::updateIfImprovement(std::shared_ptr<AlphaZeroNNGroup> trainGroup, std::shared_ptr<AlphaZeroNNGroup> generateGroup,
                                           bool doBenchmark)
{
    const std::string iterCkpt = SETTINGS.DEFAULT_CHECKPOINT_DIR + "/checkpoint-iter-" + std::to_string(trainIteration) + ".bin";
    if (SETTINGS.COMPARE_GAMES > 0) {
        const size_t samples = trainStorage.data.size();
        AlphaZeroPlayerGroup trainAZPG(trainGroup), generateAZPG(generateGroup);
        printf("Playing comparison games betweean new and old model\n");
        GameResults gr;
        if (SETTINGS.INCLUDE_COMPARE_GAMES_TRAIN_SAMPLES) {
            gr = GameGroup::playGames(trainAZPG, generateAZPG, SETTINGS.COMPARE_GAMES, &trainStorage);
            printf("New samples generated from compare games %d\n", int(trainStorage.data.size() - samples));
        } else {
            gr = GameGroup::playGames(trainAZPG, generateAZPG, SETTINGS.COMPARE_GAMES);
        }
        logFile("log/azr-improvement-log.txt") << trainIteration << ',' << gr << std::endl;
        if (isModelImproved(gr)) {
            printf("Model improved\n");
            trainGroup->saveCheckpoint(SETTINGS.DEFAULT_BEST_CHECKPOINT);
            trainGroup->saveCheckpoint(iterCkpt);
            generateGroup->loadCheckpoint(SETTINGS.DEFAULT_BEST_CHECKPOINT);
            if (doBenchmark) benchmark(generateAZPG);
            return true;
        }
        printf("Model did not improve\n");
        if (SETTINGS.TRAINING_REVERT_MODEL) {
            printf("Model reverted back old\n");
            trainGroup->loadCheckpoint(SETTINGS.DEFAULT_LATEST_CHECKPOINT);
        }
        return false;
    }
    printf("Model improved (No compare games set)\n");
    trainGroup->saveCheckpoint(SETTINGS.DEFAULT_BEST_CHECKPOINT);
    trainGroup->saveCheckpoint(iterCkpt);
    generateGroup->loadCheckpoint(SETTINGS.DEFAULT_BEST_CHECKPOINT);
    AlphaZeroPlayerGroup generateAZPG(generateGroup);
    if (doBenchmark) benchmark(generateAZPG);
    return true;
}

// ---- trainer: training without self-play (alphazero_trainer.cpp:200-317) -------------------------------------------------
void AlphaZeroTrainer::trainOnScript(std::shared_ptr<AlphaZeroNNGroup> nnGroup, std::shared_ptr<AlphaZeroNNGroup> oldNNGroup)
{
    trainStorage.loadTrainingSamples(SETTINGS.DEFAULT_SAMPLES);
    AlphaZeroPlayerGroup azpGroup(nnGroup);
    printf("Started training on script player\n");
    for (trainIteration = 0; trainIteration < SETTINGS.TRAIN_ITERATIONS; trainIteration++) {
        printf("Train iteration %ld\n", trainIteration);
        GameResults gr = GameGroup::playGames(azpGroup, AZR_PLAYER_SCRIPT, SETTINGS.TRAIN_ITERATION_GAMES * 2, &trainStorage);
        logFile("log/azr-benchmark-log.txt") << trainIteration << ",,,," << gr << std::endl;
        trainStorage.trimOldExamples();
        nnGroup->train(trainStorage.data, SETTINGS.EPOCHS);
        if (updateIfImprovement(nnGroup, oldNNGroup, false)) trainStorage.updateOldGamesIndex();
    }
    trainStorage.saveTrainingSamples(SETTINGS.DEFAULT_SAMPLES);
}

void AlphaZeroTrainer::trainOnGeneratedData(std::shared_ptr<AlphaZeroNNGroup> trainGroup, std::shared_ptr<AlphaZeroNNGroup> generatorGroup)
{
    printf("Started training on generated data\n");
    for (int e = 0; e < SETTINGS.DATA_TRAIN_LOOPS; e++) {
        printf("===> Train loop %d\n", e);
        NNTrainDataStorage storage;
        const auto t0 = std::chrono::steady_clock::now();
        int played = 0;
        if (SETTINGS.DATA_GAMES_SS > 0) {
            printf("Generating training data with Script vs Script games %d\n", SETTINGS.DATA_GAMES_SS);
            const size_t before = storage.data.size();
            const int n = GameGroup::playScripted(*trainGroup, AZR_PLAYER_SCRIPT, AZR_PLAYER_SCRIPT, SETTINGS.DATA_GAMES_SS, storage);
            if (n != SETTINGS.DATA_GAMES_SS) printf("Played %d games (whole mirrored pairs)\n", n);
            printf("Samples generated %d\n", int(storage.data.size() - before));
            played += n;
        }
        if (SETTINGS.DATA_GAMES_SR > 0) {
            printf("Generating training data with Script vs Random games: %d\n", SETTINGS.DATA_GAMES_SR);
            const size_t before = storage.data.size();
            const int n = GameGroup::playScripted(*trainGroup, AZR_PLAYER_SCRIPT, AZR_PLAYER_RANDOM, SETTINGS.DATA_GAMES_SR, storage);
            if (n != SETTINGS.DATA_GAMES_SR) printf("Played %d games (whole mirrored pairs)\n", n);
            printf("Samples generated %d\n", int(storage.data.size() - before));
            played += n;
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Generated %zu samples from %d games in %.2f s\n", storage.data.size(), played, dt);
        trainGroup->train(storage.data, 3);
        {
            printf("Playing comparison games betweean new and old model\n");
            AlphaZeroPlayerGroup azpGroup(trainGroup), oldAzpGroup(generatorGroup);
            GameResults grc = GameGroup::playGames(azpGroup, oldAzpGroup, SETTINGS.COMPARE_GAMES);
            logFile("log/azr-improvement-log.txt") << grc << std::endl;
            if (isModelImproved(grc)) {
                printf("Model improved\n");
                trainGroup->saveCheckpoint(SETTINGS.DEFAULT_CHECKPOINT_DIR + "/checkpoint-data-epoch-" + std::to_string(e) + ".bin");
                trainGroup->saveCheckpoint(SETTINGS.DEFAULT_LATEST_CHECKPOINT);
                generatorGroup->loadCheckpoint(SETTINGS.DEFAULT_LATEST_CHECKPOINT);
                printf("Playing benchmark games\n");
                GameResults grb = GameGroup::playGames(azpGroup, AZR_PLAYER_SCRIPT, SETTINGS.BENCHMARK_GAMES_SCRIPT);
                logFile("log/azr-benchmark-log.txt") << grb << std::endl;
            }
            trainGroup->saveCheckpoint(SETTINGS.DEFAULT_CHECKPOINT_TEMP);   // keep the latest model on disk at all times
        }
    }
}

}  // namespace azrhost
