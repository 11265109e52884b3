#!/usr/bin/env python3
"""Generates tests/golden/scripted_samples.npz: the records the REAL reference's ScriptPlayer / RandomPlayer push into a
train storage attached to both players (Player::addTrainingSample, player/base/player.cpp:9-17; train-data's one shared
storage, alphazero_trainer.cpp:240-275), through tests/helpers/scripted_samples_probe.cpp linked with oracle/_ref.

Run in the build container only:   python tests/golden/make_scripted_samples_golden.py

  configs        [6,4] int32   (kind0, kind1, mirror, base seed): (Script, Script), (Script, Random), (Random, Script) x
                               mirror on / off; slot g plays with seed base + g (ref_play_games, the device arena's slots)
  count          [6,3,4]       records per game (config, slot, game)
  status, rounds [6,3,4]       the game's status and round count
  digest         [N] uint64    blake2b(digest_size = 8) of every record's 265 bytes, in (config, slot, game, move) order
  full_<k0><k1>  [n,265] uint8 every record of the shortest game of that pairing (mirror on), for diagnosis
  full_at_<k0><k1> [3]         its (config, slot, game)
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AZR_REF_SRC", "/root/reference")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
PROBE = os.path.join(ROOT, "tests", "helpers", "scripted_samples_probe.cpp")
OUT = os.path.join(HERE, "scripted_samples.npz")

PAIRINGS = [(1, 1), (1, 2), (2, 1)]
SLOTS, GAMES = 3, 4
# the reference's compile switches (oracle/Makefile RULES)
RULES = ["-DINPUT_VECTOR_TYPE_2", "-DSTATE_SIMPLE_CARDS", "-DFAST_ATTACK_MOBILIZATION", "-DFAST_REINFORCEMENT"]


def configs():
    out = []
    for i, (k0, k1) in enumerate(PAIRINGS):
        for mirror in (1, 0):
            out.append((k0, k1, mirror, 7100 + 1000 * i + 100 * mirror))
    return np.array(out, np.int32)


def digest(rec):
    return np.frombuffer(hashlib.blake2b(rec.tobytes(), digest_size=8).digest(), np.uint64)[0]


def compile_probe(d):
    exe = os.path.join(d, "scripted_samples_probe")
    subprocess.check_call(["g++", "-std=gnu++2a", "-w", "-O2", "-pthread", *RULES, "-I" + os.path.join(REF, "libs"),
                           "-I" + os.path.join(REF, "src"), PROBE, "-o", exe, "-L" + REF_DIR, "-l:libazr_ref.so",
                           "-Wl,-rpath," + REF_DIR])
    return exe


def run_probe(exe, d, k0, k1, games, mirror, seed):
    """(meta [games,3] = records / status / rounds, records [n,265]) of one slot"""
    out = os.path.join(d, "slot.bin")
    subprocess.check_call([exe, str(k0), str(k1), str(games), str(mirror), str(seed), out])
    b = np.fromfile(out, np.uint8)
    ng = int(b[:4].view(np.int32)[0])
    meta = b[4:4 + 12 * ng].view(np.int32).reshape(ng, 3)
    rec = b[4 + 12 * ng:].reshape(-1, 265)
    assert len(rec) == meta[:, 0].sum()
    return meta, rec


def generate():
    cf = configs()
    count = np.zeros((len(cf), SLOTS, GAMES), np.int32)
    status = np.zeros((len(cf), SLOTS, GAMES), np.int8)
    rounds = np.zeros((len(cf), SLOTS, GAMES), np.int32)
    digests, full = [], {}
    with tempfile.TemporaryDirectory() as d:
        exe = compile_probe(d)
        for c, (k0, k1, mirror, base) in enumerate(cf):
            for g in range(SLOTS):
                meta, rec = run_probe(exe, d, k0, k1, GAMES, mirror, base + g)
                count[c, g], status[c, g], rounds[c, g] = meta[:, 0], meta[:, 1], meta[:, 2]
                digests += [digest(r) for r in rec]
                if mirror:
                    at = 0
                    for i in range(GAMES):
                        key = "%d%d" % (k0, k1)
                        if key not in full or meta[i, 0] < len(full[key][1]):
                            full[key] = ((c, g, i), rec[at:at + meta[i, 0]].copy())
                        at += meta[i, 0]
    out = dict(configs=cf, count=count, status=status, rounds=rounds, digest=np.array(digests, np.uint64))
    for key, (where, rec) in full.items():
        out["full_" + key] = rec
        out["full_at_" + key] = np.array(where, np.int32)
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("%s: %d games, %d records, %d bytes" % (OUT, out["count"].size, len(out["digest"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())
