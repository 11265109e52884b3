"""`-m play --p1 az --p2 az` with a net of its own depth and arithmetic for player 2 (--blocks2 / --dtype2).  CPU part: the flags are
listed and written to log/settings.txt, and default to --blocks / --dtype.  GPU part: a mixed arena runs to its end through the CLI, and
the command line without the new flags still plays the games it played before them — checked against the same arena played through the
binding with two handles of equal shape (same checkpoints, same seed), not against a string of the CLI's own."""
import importlib
import subprocess

import pytest

from host_cli import exe  # noqa: F401  (a fixture)



def test_help_lists_the_second_nets_flags(exe):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--blocks2", "--dtype2"):
        line = [l for l in out.split("\n") if l.strip().startswith(flag)]
        assert len(line) == 1 and "[this build]" in line[0], flag


def _settings(exe, tmp_path, *args):
    # the settings file is written before the first engine is created: it exists whether or not the run finds a device
    subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--cg", "2", "--mcts", "2", "--gpu-games", "2", *args],
                   cwd=tmp_path, capture_output=True, text=True, timeout=600)
    s = {}
    for l in open(tmp_path / "log" / "settings.txt").read().splitlines():
        name, rest = l.split("(", 1)
        s[name] = rest.rsplit(")=", 1)[1]
    return s


def test_settings_file_carries_the_second_nets_shape(exe, tmp_path):
    s = _settings(exe, tmp_path, "--blocks", "1", "--blocks2", "2", "--dtype2", "f32x")
    assert (s["blocks"], s["dtype"], s["blocks2"], s["dtype2"]) == ("1", "bf16", "2", "f32x")
    # a net of another depth cannot read player 1's checkpoint file, the default of --c2: it gets a default of its own
    assert s["c1"] == "checkpoints/latest-checkpoint.bin" and s["c2"] == "checkpoints/latest-checkpoint-2-blocks.bin"
    s = _settings(exe, tmp_path, "--blocks", "3", "--dtype", "f16")          # not given: what --blocks / --dtype say
    assert (s["blocks"], s["dtype"], s["blocks2"], s["dtype2"]) == ("3", "f16", "3", "f16")
    assert s["c1"] == s["c2"] == "checkpoints/latest-checkpoint.bin"
    r = subprocess.run([exe, "-m", "play", "--dtype2", "fp8"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "--dtype2" in r.stderr


def _tail(stdout):
    tail = stdout.strip().split("\n")[-4:]
    assert tail[0].startswith("Games: ")
    return [int(t.split(":")[1]) for t in tail]


@pytest.mark.gpu
def test_play_mode_between_nets_of_different_depth_and_arithmetic(exe, tmp_path):
    r = subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--blocks", "1", "--blocks2", "2", "--dtype2", "f32x",
                        "--mcts", "8", "--cg", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    games, d, p1, p2 = _tail(r.stdout)
    assert games == 8 and d + p1 + p2 == 8


@pytest.mark.gpu
def test_play_mode_without_the_new_flags_plays_the_equal_shape_arena(exe, tmp_path):
    """the old command line: both groups --blocks 1, bf16.  The same arena through the binding — two equal handles with the checkpoints
    the CLI wrote, GameGroup::playGames' seed of its first call (base + 7919), the same slots and threads — gives the result"""
    r = subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--blocks", "1", "--mcts", "8", "--cg", "8", "--gpu-games", "8", "-t", "2",
                        "--c2", "checkpoints/second.bin"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    games, d, p1, p2 = _tail(r.stdout)
    P = importlib.import_module("alphazero-risk_amd")
    a = P.Engine(8, blocks=1, sims=8, dtype=P.NET_BF16, threads=2)          # every other setting: the C default = the CLI's default
    b = P.Engine(8, blocks=1, sims=8, dtype=P.NET_BF16, threads=2)
    a.load(str(tmp_path / "checkpoints" / "latest-checkpoint.bin"))        # written by the CLI (a missing checkpoint is initialised and saved)
    b.load(str(tmp_path / "checkpoints" / "second.bin"))
    a.arena_set_opponent(b)
    a.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 8, 0, P.MIRROR_CONCURRENT, 20260001 + 7919)   # --seed's default + the first call's offset
    while not a.arena_run(64):
        pass
    res = a.arena_results()
    a.arena_set_opponent(None)
    a.close(); b.close()
    assert [games, d, p1, p2] == [res["count"], res["draw"], res["win"][0], res["win"][1]]
