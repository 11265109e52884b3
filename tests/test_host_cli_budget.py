"""`-m play --p1 az --p2 az` with a search budget of its own for player 2 (--mcts2 / --hp2).  CPU part: the flags are listed, written to
log/settings.txt with the value in force, a value that is no budget is rejected, and without them the start line is the one the CLI
printed before they existed.  GPU part: an arena of 8 simulations against 2 runs to its end through the CLI."""
import subprocess

import pytest

from host_cli import exe  # noqa: F401  (a fixture)


# what the CLI built from the commit before --mcts2 / --hp2 printed first for ARGS (Settings::describe, recorded from that build)
ARGS = ["-m", "play", "--p1", "az", "--p2", "az", "--mcts", "8", "--blocks", "1", "--blocks2", "1", "--cg", "4", "--gpu-games", "6", "-t", "2"]
START_LINE = "===> Starting program with GPUs: 1, Games per GPU 6, MCTS threads: 2, MCTS simulations 8"


def _settings(tmp_path):
    s = {}
    for l in open(tmp_path / "log" / "settings.txt").read().splitlines():
        name, rest = l.split("(", 1)
        s[name] = rest.rsplit(")=", 1)[1]
    return s


def test_help_lists_the_second_players_search_flags(exe):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag, dflt in (("--mcts2", "--mcts"), ("--hp2", "--hp")):
        line = [l for l in out.split("\n") if l.strip().startswith(flag + " ")]
        assert len(line) == 1 and "[this build]" in line[0] and "(default: %s)" % dflt in line[0], flag


def test_a_value_that_is_no_budget_is_rejected(exe, tmp_path):
    for flag, value in (("--mcts2", "many"), ("--mcts2", "0"), ("--mcts2", "8x"), ("--mcts2", "1"), ("--hp2", "high")):
        r = subprocess.run([exe, "-m", "play", flag, value], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and flag in r.stderr and value in r.stderr, (flag, value, r.stderr)
        assert "Starting program" not in r.stdout
    r = subprocess.run([exe, "-m", "play", "--mcts3", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "does not exist" in r.stderr


def test_without_the_flags_the_start_line_is_unchanged(exe, tmp_path):
    # the line is printed, and the settings file written, before the first engine is created: with or without a device
    def played_or_found_no_device(r):   # nothing else may end the run: not a crash, not a rejected flag
        return (r.returncode == 0 and "Games: 4" in r.stdout) or (r.returncode == 1 and r.stderr.startswith("fatal: engine: hip"))

    r = subprocess.run([exe, *ARGS], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.stdout.split("\n")[0] == START_LINE and played_or_found_no_device(r), (r.returncode, r.stderr)
    s = _settings(tmp_path)
    assert (s["mcts"], s["mcts2"]) == ("8", "8") and s["hp"] == s["hp2"]          # not given: what --mcts / --hp say
    r = subprocess.run([exe, *ARGS, "--mcts2", "2", "--hp2", "2.5"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.stdout.split("\n")[0] == START_LINE and played_or_found_no_device(r), (r.returncode, r.stderr)   # describe(): player 1's search
    s = _settings(tmp_path)
    assert (s["mcts"], s["mcts2"], s["hp2"]) == ("8", "2", "2.5") and float(s["hp"]) == pytest.approx(1.1)


@pytest.mark.gpu
def test_play_mode_with_a_budget_per_side(exe, tmp_path):
    r = subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--mcts", "8", "--mcts2", "2", "--blocks", "1", "--blocks2", "1",
                        "--cg", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    tail = r.stdout.strip().split("\n")[-4:]
    assert tail[0] == "Games: 4"
    d, p1, p2 = (int(t.split(":")[1]) for t in tail[1:])
    assert d + p1 + p2 == 4
    # the larger budget on player 2: the engines are created with room for it
    r = subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--mcts", "2", "--mcts2", "8", "--hp2", "2.0", "--blocks", "1",
                        "--blocks2", "1", "--cg", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert r.stdout.strip().split("\n")[-4] == "Games: 4"
