"""The value mix of the self-play records, restated from include/azr.h in np.float32, operation for operation (TEST INFRASTRUCTURE):
the root value q of a finished search and the blend of a record's outcome z with it.  Every float operation below is one fp32
operation of the header, rounded on its own, in the header's order.

tests/test_value_mix_ref.py checks the restatement against float64 on the CPU; tests/test_gpu_value_mix.py pins the device to it bit
for bit."""
import numpy as np

from azr_testlib import bits

f32 = np.float32
MOVES = 43


def root_sums(N, Q, valid):
    """(num, den) of one root: N uint32 [43], Q float32 [43], valid the legal-move mask"""
    N, Q, ok = np.asarray(N, np.uint32), np.asarray(Q, f32), bits(valid)
    num, den = f32(0.0), f32(0.0)
    for m in range(MOVES):
        if ok[m] and N[m] > 0:
            n = f32(N[m])
            num = f32(num + f32(n * Q[m]))
            den = f32(den + n)
    return num, den


def root_value(N, Q, valid):
    """(q float32, has_q bool) of one root; q = 0 without has_q"""
    num, den = root_sums(N, Q, valid)
    if not den > 0:
        return f32(0.0), False
    q = f32(num / den)
    return f32(min(max(q, f32(-1.0)), f32(1.0))), True


def blend(z, q, has_q, q_share):
    """z' of a record with the outcome z and the root value q"""
    z, q, s = f32(z), f32(q), f32(q_share)
    if not has_q:
        return z
    a = f32(f32(1.0) - s)
    b = f32(f32(a * z) + f32(s * q))
    return f32(min(max(b, f32(-1.0)), f32(1.0)))


def mix_rows(q_share, N, Q, valid, z):
    """the rule on rows: N, Q [rows, 43], valid, z [rows] -> (q float32, has_q bool, z' float32), each [rows]"""
    rows = len(z)
    q, has, zz = np.zeros(rows, f32), np.zeros(rows, bool), np.zeros(rows, f32)
    for i in range(rows):
        q[i], has[i] = root_value(N[i], Q[i], valid[i])
        zz[i] = blend(z[i], q[i], has[i], q_share)
    return q, has, zz
