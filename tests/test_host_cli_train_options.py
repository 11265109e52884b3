"""The C++ host's flags of the optimiser step's options (a table of their own in Settings::init): listed by --help, carried into
log/settings.txt, and refused — before an engine exists — where azr_nn_train_set_options would refuse them.  No device needed."""
import pytest

from host_cli import check_defaults, check_flags_carried, check_host_rejects, exe, learn_records  # noqa: F401  (exe: the fixture)

FLAGS = ["--lr", "--l2", "--lr-schedule", "--lr-warmup", "--lr-steps", "--lr-min", "--lr-period", "--lr-gamma", "--clip-norm", "--ema-decay", "--ema-play"]


def test_flags_are_listed_and_carried(exe, tmp_path):  # noqa: F811
    check_flags_carried(exe, tmp_path, FLAGS, ["0.0003", "0", "cosine", "3", "6", "0.00003", "4", "0.5", "1", "0.999", "1"])


def test_defaults_are_the_reference_step(exe, tmp_path):  # noqa: F811
    check_defaults(exe, tmp_path, FLAGS, ["0.001", "0.001", "constant", "0", "0", "0", "1", "1", "0", "0", "0"])


def test_refused_values(exe, tmp_path):  # noqa: F811
    for args, flag in ((["--lr", "0"], "--lr"), (["--lr=nan"], "--lr"), (["--l2=-0.1"], "--l2"), (["--lr-schedule", "linear"], "--lr-schedule"),
                       (["--lr-warmup=-1"], "--lr-warmup"), (["--lr-schedule", "cosine", "--lr-warmup", "5", "--lr-steps", "5"], "--lr-steps"),
                       (["--lr-schedule", "cosine", "--lr-steps", "5", "--lr-min", "0.01"], "--lr-min"), (["--lr-period", "0"], "--lr-period"),
                       (["--lr-gamma", "0"], "--lr-gamma"), (["--lr-gamma", "1.5"], "--lr-gamma"), (["--clip-norm=-1"], "--clip-norm"),
                       (["--clip-norm", "inf"], "--clip-norm"), (["--ema-decay", "1"], "--ema-decay"), (["--ema-play", "1"], "--ema-play"),
                       (["--ema-play", "2", "--ema-decay", "0.9"], "--ema-play")):
        check_host_rejects(exe, tmp_path, args, flag)


@pytest.mark.gpu
def test_learn_iteration_with_the_options_on(exe, tmp_path):  # noqa: F811
    """one learn iteration with clipping, a schedule and the averaged net playing: the training phase logs its optimiser line, the
    compare games and the checkpoint take the EMA weights (azr_nn_get_ema_weights -> azr_nn_set_weights) and the run ends clean"""
    run = learn_records(exe, str(tmp_path / "run"), "--clip-norm=0.5", "--lr-schedule=step", "--lr-period=1", "--lr-gamma=0.5", "--ema-decay=0.5",
                        "--ema-play=1", tg=4)
    line = [l for l in run.stdout.splitlines() if l.startswith("Optimiser step: lr ")]
    assert len(line) == 1 and line[0].endswith("[the averaged net plays]") and "grad norm n/a" not in line[0], run.stdout[-2000:]
    assert "Model improved" in run.stdout
