"""The C++ host's --dir-alpha / --dir-seed: sampled root noise in the self-play generation of `-m learn`.  CPU part: the flags are
listed, written to log/settings.txt and a value that is no Dirichlet parameter is rejected.  GPU part: a learn iteration with noise
runs to its end, its samples are a function of --dir-seed, and --dir-alpha 0 is the run without the flags."""
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, ("--dir-alpha", "--dir-seed"), ("0.3", "7"))


@pytest.mark.parametrize("bad", ["-1", "10.5", "nan", "x"])
def test_a_value_that_is_no_dirichlet_parameter_is_rejected(exe, tmp_path, bad):
    H.check_host_rejects(exe, tmp_path, ["--dir-alpha=" + bad], "--dir-alpha")


@pytest.mark.gpu
def test_learn_with_root_noise_is_a_function_of_dir_seed(exe, tmp_path):
    a = H.learn_records(exe, tmp_path / "a", "--dir-alpha", "0.3", "--dir-seed", "7").raw
    b = H.learn_records(exe, tmp_path / "b", "--dir-alpha", "0.3", "--dir-seed", "7").raw
    c = H.learn_records(exe, tmp_path / "c", "--dir-alpha", "0.3", "--dir-seed", "8").raw
    assert a == b
    assert a != c


@pytest.mark.gpu
def test_dir_alpha_zero_is_the_run_without_the_flags(exe, tmp_path):
    off = H.learn_records(exe, tmp_path / "off", "--dir-alpha", "0", "--dir-seed", "7").raw
    absent = H.learn_records(exe, tmp_path / "absent").raw
    assert off == absent
