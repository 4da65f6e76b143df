"""The C++ side of the harnesses' typed-array files (tools/kbench_io.h: read_launch, write_arrays) on the CPU: tools/kbench_io_echo.cpp, compiled
with the host compiler, reads one real case of each of the five helpers that use the format and writes every array back with 64 guard entries;
malformed files must be refused with exit status 2 and leave no result.  The Python side is tests/helpers/harness_io.py."""
import os, shutil, struct, subprocess
import numpy as np
import pytest
from tests.helpers import harness_io as IO
from tests.helpers import adapt_cases as A, dense_cases as D, mfma_cases as M, rollout_cases as RC, loop_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 28                                                # the tools' limit on one array's count (kbench_loop: 1 << 26)
MAGIC_OUT = b"ECHORES1"


@pytest.fixture(scope="module")
def echo(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("echo") / "kbench_io_echo")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tools", "kbench_io_echo.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return exe


def _echo(exe, tmp_path, data, magic, multi=False, max_type=2, max_arrays=16, max_B=8, cap=CAP):
    """-> (exit status, the result file's bytes or None)"""
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(fin, "wb") as f:
        f.write(data)
    if os.path.exists(fout):
        os.remove(fout)
    r = subprocess.run([exe, fin, fout, magic.decode(), MAGIC_OUT.decode(), str(int(multi)), str(max_type), str(max_arrays), str(max_B), str(cap)],
                       capture_output=True, text=True, timeout=60)
    return r.returncode, (open(fout, "rb").read() if os.path.exists(fout) else None)


def _check_arrays(sent, got):
    assert len(sent) == len(got)
    for (t, a), (tg, g) in zip(sent, got):
        body, guard = IO.split_guard(g, (a.size,))
        assert tg == t and body.tobytes() == a.tobytes() and np.all(IO.is_poison(guard)), t


SINGLE = [("adapt", lambda: A.update_case(17, True, False, False)["data"], A.MAGIC_IN, 1), ("dense", lambda: D.solve_case(5, "graded", False, True, True, True)["data"], D.MAGIC_IN, 2),
          ("mfma", lambda: M.wcov_case(17, 65, 2, "w")["data"], M.MAGIC_IN, 2)]


@pytest.mark.parametrize("name,make,magic,max_type", SINGLE, ids=[s[0] for s in SINGLE])
def test_single_launch_case_comes_back_bit_for_bit(echo, tmp_path, name, make, magic, max_type):
    data = make()
    rc, res = _echo(echo, tmp_path, data, magic, max_type=max_type)
    assert rc == 0 and res is not None
    (form, guard, n), got = IO.unpack_arrays(MAGIC_OUT, 3, res)
    sent = IO.unpack_case(magic, data)[4]
    assert (form, guard, n) == (0, IO.GUARD, len(sent)) and any(t != IO.F64 for t, _ in sent)
    _check_arrays(sent, got)


def _multi():
    L = RC.car_launch(2, 2, 5, 3, 1, traj=True, iters=True, cmin=np.array([1, 2], dtype=np.uint64))
    yield "rollout", RC.pack([L, RC.copy_launch(7, 2)]), RC.MAGIC_IN, 16, 8
    rows = [np.linspace(0.0, 1.0, 9), np.linspace(1.0, 0.0, 9)]
    yield "loop", LC.pack([LC.plan_launch(9, 3, 4, rows, 5)] + LC.reorder_launches()[:2]), LC.MAGIC_IN, 24, 256


@pytest.mark.parametrize("name,data,magic,max_arrays,max_B", list(_multi()), ids=["rollout", "loop"])
def test_multi_launch_case_comes_back_bit_for_bit(echo, tmp_path, name, data, magic, max_arrays, max_B):
    rc, res = _echo(echo, tmp_path, data, magic, multi=True, max_arrays=max_arrays, max_B=max_B)
    assert rc == 0 and res is not None
    assert res[:8] == MAGIC_OUT and data[:8] == magic
    guard, nL = struct.unpack_from("<2q", res, 8)
    assert guard == IO.GUARD and nL == struct.unpack_from("<q", data, 8)[0] >= 2
    off_in, off = 16, 24
    for _ in range(nL):
        (op, B, ipar, dpar, sent), off_in = IO.unpack_launch(data, off_in)
        rop, nA = struct.unpack_from("<2q", res, off)
        off += 16
        got = []
        for _ in range(nA):
            t, a, off = IO.unpack_array(res, off)
            got.append((t, a))
        assert rop == op
        _check_arrays(sent, got)
    assert off_in == len(data) and off == len(res)


def _small():
    """a well-formed single-launch case: 3 ipar, 2 dpar, arrays f64[5], i32[3], not given, u64[2]"""
    arrays = [(IO.F64, np.arange(5.0)), (IO.I32, np.array([1, 0, 1])), (IO.F64, None), (IO.U64, np.array([7, 1 << 63], dtype=np.uint64))]
    return IO.pack_case(b"TESTCASE", 2, 3, [4, 5, 6], [0.5, -1.0], arrays)


def _set_word(data, off, v):
    return data[:off] + struct.pack("<q", v) + data[off + 8:]


# offsets in _small(): magic 0, record header 8..48, ipar 48..72, dpar 72..88, array 0 header 88 (type) / 96 (count), its data 104..144, array 1 header 144
MALFORMED = [("cut inside the header", lambda d: d[:30]), ("cut inside ipar", lambda d: d[:60]), ("cut inside an array", lambda d: d[:120]),
             ("cut inside an array header", lambda d: d[:150]), ("wrong magic", lambda d: b"TESTCASF" + d[8:]), ("negative count", lambda d: _set_word(d, 96, -1)),
             ("count above the cap", lambda d: _set_word(d, 96, CAP + 1)), ("array type above the limit", lambda d: _set_word(d, 88, 3)),
             ("array type below zero", lambda d: _set_word(d, 88, -1)), ("one trailing byte", lambda d: d + b"\0"), ("B above the limit", lambda d: _set_word(d, 16, 9)),
             ("more arrays than the tool takes", lambda d: _set_word(d, 40, 17)), ("negative n_ipar", lambda d: _set_word(d, 24, -1)), ("empty file", lambda d: b"")]


def test_the_small_case_is_accepted_and_at_the_limits_too(echo, tmp_path):
    d = _small()
    assert struct.unpack_from("<q", d, 96)[0] == 5 and struct.unpack_from("<q", d, 88)[0] == IO.F64 and struct.unpack_from("<q", d, 144)[0] == IO.I32
    rc, res = _echo(echo, tmp_path, d, b"TESTCASE")
    assert rc == 0
    _check_arrays(IO.unpack_case(b"TESTCASE", d)[4], IO.unpack_arrays(MAGIC_OUT, 3, res)[1])
    assert _echo(echo, tmp_path, _set_word(d, 16, 8), b"TESTCASE")[0] == 0                    # B at its limit
    assert _echo(echo, tmp_path, d, b"TESTCASE", cap=5)[0] == 0                               # a count at the cap
    assert _echo(echo, tmp_path, d, b"TESTCASE", cap=4) == (2, None)                          # and one above


@pytest.mark.parametrize("what,spoil", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_case_is_refused_and_leaves_no_result(echo, tmp_path, what, spoil):
    assert _echo(echo, tmp_path, spoil(_small()), b"TESTCASE") == (2, None), what


def test_type_limit_of_the_two_type_tools_and_truncated_multi_launch_files(echo, tmp_path):
    d = _small()
    assert _echo(echo, tmp_path, d, b"TESTCASE", max_type=1) == (2, None)                     # the u64 array: kbench_adapt takes f64 and i32 only
    multi = IO.pack_launches(b"TESTCASE", [d[8:], d[8:]])
    assert _echo(echo, tmp_path, multi, b"TESTCASE", multi=True)[0] == 0
    for bad in (multi[:-1], multi + b"\0", _set_word(multi, 8, 3), _set_word(multi, 8, 0), multi[:12]):
        assert _echo(echo, tmp_path, bad, b"TESTCASE", multi=True) == (2, None)
