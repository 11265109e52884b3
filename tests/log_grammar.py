"""The grammar of the learn loop's three log files (TEST INFRASTRUCTURE): written once here, checked against every line the reference
ever wrote by tests/test_log_grammar.py, and applied to the files the learn loop and the host CLI leave behind.  Fixtures: the authors'
own log files (tests/golden/ref_logs.json, output data of their runs)."""
import csv
import io
import json
import os
import re

import azr_testlib as T

REF = json.load(open(os.path.join(T.GOLDEN, "ref_logs.json")))   # the authors' own log files (tests/golden/make_logs_golden.py)


def ref_text(kind):
    return REF[kind]["text"]


def ref_first_line(kind):
    return REF[kind]["text"].split("\n")[0] + "\n"


PLAYER = r"\d+/\d+"
GR = rf"\d+, {PLAYER}, {PLAYER}"                       # operator<<(GameResults), game.cpp:227-235: draw, W/Wstart, W/Wstart
IMPROVEMENT = re.compile(rf"^\d+,{GR}$")                # alphazero_trainer.cpp:163
BENCHMARK = re.compile(rf"^\d+,{GR}, {GR}$")            # alphazero_trainer.cpp:139
FLOAT = r"-?(?:\d+\.?\d*|\.\d+)(?:e[-+]?\d+)?|nan|inf"
NN_TRAINING = re.compile(rf"^(?:(?:{FLOAT}), (?:{FLOAT}), ?)*$")  # "policy, value, " per epoch (some of the authors' lines lost the last blank)


def chart_parse(kind, text):
    """what python/src/log_chart.py does with a file (its csv.reader + int/split logic), returning the parsed rows"""
    rows = []
    for row in csv.reader(io.StringIO(text), delimiter=","):
        if kind == "improvement":      # GameResults(row)
            rows.append((int(row[0]), int(row[1])) + tuple(int(x) for x in row[2].split("/")) + tuple(int(x) for x in row[3].split("/")))
        elif kind == "benchmark":      # GameResults(row[0:4]), GameResults(row[0:1] + row[4:])
            assert len(row) == 7
            rows.append((int(row[0]), int(row[1]), int(row[4])) + tuple(int(x) for f in (row[2], row[3], row[5], row[6]) for x in f.split("/")))
        else:                          # float(row[0]), float(row[1]), ... ; the trailing ", " leaves one blank field
            assert not row or row[-1].strip() == ""      # (an empty line = a train() call with fewer records than one batch)
            rows.append(tuple(float(x) for x in row[:-1]))
    return rows


def check(kind, text, complete=True):
    rx = {"improvement": IMPROVEMENT, "benchmark": BENCHMARK, "nn": NN_TRAINING}[kind]
    lines = text.split("\n")
    if complete:
        assert lines[-1] == "", "file ends with a newline"
    else:   # the authors' NN log stops in the middle of a train() call: its last line has no newline yet
        assert rx.match(lines[-1])
    for ln in lines[:-1]:
        assert rx.match(ln.rstrip(" ") if kind != "nn" else ln), (kind, ln)
    return chart_parse(kind, text)
