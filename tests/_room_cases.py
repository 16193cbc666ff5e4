"""Rooms, jobs and references shared by tests/test_room.py and tests/test_gpu_room.py (not a test module)."""
import ctypes as C
import functools

import numpy as np

RATE = 8000
C_SOUND = 343.0
SIX = (0.9, 0.7, 0.8, 0.85, 0.6, 0.95)          # six different walls

# CPU cases of the restatement and its faults: (L, beta, src, mic, ntaps).  Every wall reflects and the two walls of an axis
# differ, so that a lost parity class, a lost outer shell, a shifted tap and a wrong exponent all change the result.
F32_CASES = [
    ((3.1, 2.6, 2.3), SIX, (1.1, 0.9, 1.3), (2.2, 1.7, 0.8), 700),
    ((2.2, 2.0, 2.1), (0.95, 0.9, 0.95, 0.9, 0.95, 0.9), (0.7, 1.2, 1.0), (1.6, 0.6, 1.3), 700),
    ((6.0, 5.0, 3.0), (0.97, 0.95, 0.85, 0.8, 0.8, 0.75), (1.1, 2.3, 1.5), (3.7, 2.9, 1.2), 2400),     # (the long axis' walls reflect most:
                                                                                                    #  its outermost shell is not lost in the tail)
    ((4.0, 3.0, 2.5), SIX, (1.0, 1.0, 1.0), (3.1, 2.2, 1.4), 257),
]
FAULTS = [dict(drop_parity=5), dict(drop_outer_axis=0), dict(tap_shift=1), dict(same_exponent=True)]

D40 = 40.0 * C_SOUND / RATE                      # a direct path of exactly 40 samples


def _eyring(L, t60):
    from sepkern import room
    return tuple(room.eyring_beta(L, t60))


# The GPU launch: (L, beta, src, mic, ntaps, scale) -- what each job is there for is in tests/test_gpu_room.py's docstring.
def gpu_jobs():
    return [
        ((5.0, 4.0, 3.0), (0.5,) * 6, (2.0, 2.0, 1.5), (2.02, 2.0, 1.5), 1, 1.0),
        ((5.0, 4.0, 3.0), (0.0,) * 6, (2.0, 2.0, 1.5), (2.0, 2.02, 1.5), 33, 1.0),
        ((5.0, 4.0, 3.0), (0.8,) * 6, (1.0, 2.0, 1.5), (4.0, 2.0, 1.5), 33, 1.0),
        ((4.0, 3.0, 2.5), (0.0, 0.9, 0.9, 0.9, 0.9, 0.0), (1.0, 1.0, 1.0), (3.1, 2.2, 1.4), 256, 1.0),
        ((3.1, 2.6, 2.3), (0.95,) * 6, (1.1, 0.9, 1.3), (2.2, 1.7, 0.8), 257, 1.0),
        ((2.2, 2.0, 2.1), (0.95,) * 6, (0.7, 1.2, 1.0), (1.6, 0.6, 1.3), 700, 1.0),
        ((3.1, 2.6, 2.3), SIX, (2.2, 1.7, 0.8), (1.1, 0.9, 1.3), 700, 4.0 * np.pi * 1.5),
        ((12.0, 10.0, 4.0), _eyring((12.0, 10.0, 4.0), 0.5), (2.0, 3.0, 1.2), (9.5, 7.0, 2.0), 4097, 1.0),
        ((6.0, 5.0, 3.0), (0.93, 0.88, 0.93, 0.88, 0.93, 0.88), (1.1, 2.3, 1.5), (3.7, 2.9, 1.2), 4097, 1.0),
        ((10.0, 8.0, 4.0), (0.95,) * 6, (2.5, 3.0, 1.6), (7.0, 5.5, 1.4), 8192, 1.0),
        ((5.0, 4.0, 3.0), (0.0,) * 6, (1.0, 1.0, 1.0), (1.0 + D40, 1.0, 1.0), 256, 4.0 * np.pi * D40),
    ]


@functools.lru_cache(maxsize=None)
def gpu_reference(j):
    """Job j -> (ism_rir fp64, the gate 2 max(e32[n], u[n]) per tap, e32 / u at its worst tap, images).  e32 is ism_rir_f32's own
    error: the yardstick is numpy's arithmetic, never the kernel's.  Computed once, shared, never written to."""
    from sepkern import room
    L, beta, src, mic, ntaps, scale = gpu_jobs()[j]
    want, u = room.ism_rir(L, beta, src, mic, RATE, ntaps, scale, want_unit=True)
    e32 = np.abs(room.ism_rir_f32(L, beta, src, mic, RATE, ntaps, scale).astype(np.float64) - want)
    gate = 2.0 * np.maximum(e32, u)
    for a in (want, gate):
        a.setflags(write=False)
    return want, gate, float(np.max(e32[u > 0] / u[u > 0])) if np.any(u > 0) else 0.0, room.count_images(L, beta, src, mic, RATE, ntaps)


def host_arrays(jobs, offs=None):
    """The host arrays of sk_room_rirs / sk_room_workspace_bytes for `jobs` (kept alive by the returned dict)."""
    J = len(jobs)
    dbl = lambda rows, w: np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(J, w))  # noqa: E731
    a = {"room": dbl([j[0] for j in jobs], 3), "beta": dbl([j[1] for j in jobs], 6), "src": dbl([j[2] for j in jobs], 3),
         "mic": dbl([j[3] for j in jobs], 3), "scale": dbl([[j[5]] for j in jobs], 1)}
    if offs is None:
        offs, at = [], 0
        for j in jobs:
            offs.append(at)
            at += max(int(j[4]), 0)
    a["ntaps"] = (C.c_int32 * J)(*[int(j[4]) for j in jobs])
    a["offs"] = (C.c_int64 * J)(*offs)
    return a


def entry_args(a, J, rate, ws=None, rir=None, stream=None, null=()):
    """-> (arguments of sk_room_workspace_bytes, arguments of sk_room_rirs); `null`: names of host arrays passed as NULL."""
    p = lambda k: None if k in null else (a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k])  # noqa: E731
    head = [p("room"), p("beta"), p("src"), p("mic"), p("scale"), p("ntaps"), p("offs"), J, float(rate)]
    return head, head + [ws, rir, stream]


GOOD = ((5.0, 4.0, 3.0), (0.5,) * 6, (2.0, 2.0, 1.5), (3.0, 2.0, 1.5), 700, 1.0)


def bad_jobs():
    """(job, rate, what sk_last_error must say) for every refusal the entry point owes."""
    L, b, s, m, n, sc = GOOD
    return [((L, b, s, m, 0, sc), RATE, b"ntaps outside"), ((L, b, s, m, 8193, sc), RATE, b"ntaps outside"),
            (((5.0, 0.0, 3.0), b, s, m, n, sc), RATE, b"room dimension"), (((5.0, 4.0, -3.0), b, s, m, n, sc), RATE, b"room dimension"),
            ((L, (0.5, 0.5, 1.01, 0.5, 0.5, 0.5), s, m, n, sc), RATE, b"reflection coefficient"),
            ((L, (0.5, -0.1, 0.5, 0.5, 0.5, 0.5), s, m, n, sc), RATE, b"reflection coefficient"),
            ((L, b, (5.0, 2.0, 1.5), m, n, sc), RATE, b"strictly inside"), ((L, b, s, (3.0, 0.0, 1.5), n, sc), RATE, b"strictly inside"),
            ((L, b, s, (2.005, 2.0, 1.5), n, sc), RATE, b"less than 0.01 m"),
            ((L, b, s, m, n, sc), 0.5, b"rate"), ((L, b, s, m, n, float("inf")), RATE, b"scale"),
            (((0.05, 0.05, 0.05), b, (0.02, 0.02, 0.02), (0.04, 0.04, 0.04), 8192, sc), RATE, b"candidate images")]


def check_refusals(lib):
    """Every SK_EINVAL case of sk_room_rirs: -1 with its message, before anything could be launched (no device pointer is ever
    given), and sk_room_workspace_bytes returns 0 for it."""
    for job, rate, word in bad_jobs():
        for jobs in ([job], [GOOD, job]):
            a = host_arrays(jobs)
            q, r = entry_args(a, len(jobs), rate)
            assert lib.sk_room_workspace_bytes(*q) == 0, (job, rate)
            assert lib.sk_room_rirs(*r) == -1 and word in lib.sk_last_error(), (job, rate, lib.sk_last_error())
    a = host_arrays([GOOD], offs=[-1])
    q, r = entry_args(a, 1, RATE)
    assert lib.sk_room_workspace_bytes(*q) == 0 and lib.sk_room_rirs(*r) == -1 and b"negative output offset" in lib.sk_last_error()
    a = host_arrays([GOOD])
    for J, word in ((0, b"J = 0"), (65536, b"J = 65536"), (-1, b"J = -1")):
        q, r = entry_args(a, J, RATE)
        assert lib.sk_room_workspace_bytes(*q) == 0 and lib.sk_room_rirs(*r) == -1 and word in lib.sk_last_error()
    for k in ("room", "beta", "src", "mic", "scale", "ntaps", "offs"):
        q, r = entry_args(a, 1, RATE, null=(k,))
        assert lib.sk_room_workspace_bytes(*q) == 0 and lib.sk_room_rirs(*r) == -1 and b"job arrays" in lib.sk_last_error()
    # good jobs, no device pointers: the last check; the workspace is the job table
    q, r = entry_args(a, 1, RATE)
    assert lib.sk_room_workspace_bytes(*q) == 256 and lib.sk_room_rirs(*r) == -1 and b"null pointer" in lib.sk_last_error()


def array3():
    """A 3-microphone array, 5 cm and 8 cm from the first."""
    return np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.08, 0.0]])
