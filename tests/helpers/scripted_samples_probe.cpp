// TEST INFRASTRUCTURE — harness glue written for this repo, in the style of oracle/ref_harness.cpp; not product code.
//
// Records what the REAL reference's ScriptPlayer / RandomPlayer push into a train storage (Player::addTrainingSample,
// player/base/player.cpp:9-17) when one NNTrainDataStorage is attached to both players, as trainOnGeneratedData does
// (alphazero_trainer.cpp:240-275).  Per slot it does exactly what ref_play_games does — seed the global engine, one Game
// with two fresh players, playGames(1) repeated — so a slot's games are those of tests/test_gpu_arena.py's slots.
//
// Built by tests/golden/make_scripted_samples_golden.py against the reference's headers, linked with oracle/_ref/libazr_ref.so
// (the reference's TF-free units, compiled there by oracle/Makefile); nothing of it is committed.
//
//   scripted_samples_probe <kind0> <kind1> <games> <mirror> <seed> <out.bin>
//     kinds: 1 = ScriptPlayer, 2 = RandomPlayer
//     out.bin: int32 games, then per game {int32 records, int32 status, int32 rounds}, then every record in the 265-byte
//              on-disk layout (i8 player | 88 B NNInputData | f32 z | f32 pi[43]), in storage order; NNInputData's padding
//              bytes (43, 46, 47) as zero, as the device writes them
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "risk_game/game/game.h"
#include "risk_game/player/random/random_player.h"
#include "risk_game/player/script/script_player.h"

extern "C" int ref_play_games(int kind0, int kind1, int games, int mirror, uint32_t seed, int* results6, int8_t* status,
                              uint8_t* finals160, uint16_t* rounds, uint32_t* rng_state);

static_assert(sizeof(NNInputData) == 88, "reference NNInputData layout changed");

int main(int argc, char** argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: %s kind0 kind1 games mirror seed out.bin\n", argv[0]);
        return 2;
    }
    const int kind0 = atoi(argv[1]), kind1 = atoi(argv[2]), games = atoi(argv[3]), mirror = atoi(argv[4]);
    const uint32_t seed = (uint32_t)strtoul(argv[5], nullptr, 10);
    // zero games through the library's own entry: sets SETTINGS.MIRROR_GAMES and seeds the global engine in the library,
    // where the players and Game draw from
    int r6[6];
    if (ref_play_games(kind0, kind1, 0, mirror, seed, r6, nullptr, nullptr, nullptr, nullptr)) return 1;
    auto mk = [](int kind) -> std::shared_ptr<Player> {
        if (kind == 1) return std::shared_ptr<Player>(new ScriptPlayer());
        return std::shared_ptr<Player>(new RandomPlayer());
    };
    NNTrainDataStorage tds;
    std::shared_ptr<Player> p0 = mk(kind0), p1 = mk(kind1);
    p0->setTrainStorage(&tds);
    p1->setTrainStorage(&tds);
    Game game;
    game.addPlayer(p0);
    game.addPlayer(p1);
    std::vector<int32_t> meta;
    size_t before = 0;
    try {
        for (int i = 0; i < games; i++) {
            game.playGames(1);
            meta.push_back((int32_t)(tds.data.size() - before));
            meta.push_back((int32_t)game.state.gameStatus());
            meta.push_back((int32_t)game.state.getRound());
            before = tds.data.size();
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    FILE* f = fopen(argv[6], "wb");
    if (!f) return 1;
    const int32_t ng = games;
    fwrite(&ng, 4, 1, f);
    fwrite(meta.data(), 4, meta.size(), f);
    uint8_t rec[265];
    for (const NNTrainData& d : tds.data) {
        rec[0] = (uint8_t)d.playerIndex;
        std::memcpy(rec + 1, (const void*)&d.in, 88);
        rec[1 + 43] = rec[1 + 46] = rec[1 + 47] = 0;   // NNInputData's struct padding, which the reference leaves unset
        std::memcpy(rec + 89, &d.out.value, 4);
        std::memset(rec + 93, 0, 172);
        std::memcpy(rec + 93, d.out.policy.data(), 4 * std::min<size_t>(43, d.out.policy.size()));
        fwrite(rec, 1, 265, f);
    }
    fclose(f);
    return 0;
}
