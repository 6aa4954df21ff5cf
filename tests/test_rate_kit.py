"""tools/rate_kit.py without a GPU: the alternation of forms under a scripted clock, the printed row, the command line, and the
alternation of two builds in fresh processes against a stub child script."""
import subprocess
import sys
import textwrap

import pytest

import rate_kit  # tools/ is on sys.path (conftest)


class Clock:
    """a clock that records (form, iters) and answers the form's scripted per-call ms"""
    def __init__(self, ms, log):
        self.ms, self.log = ms, log

    def __call__(self, fn, iters):
        self.log.append(("clock", fn.__name__, iters))
        return self.ms[fn.__name__].pop(0)


def form(name, log):
    def fn():
        log.append(("call", name))
    fn.__name__ = name
    return fn


def test_alternate_warms_up_sizes_takes_turns_and_sorts():
    log = []
    sizing = {"a": 0.0005, "b": 3.0, "c": 40.0, "d": 500.0}
    scripted = {"a": [3.0, 1.0, 2.0], "b": [9.0, 8.0, 7.0], "c": [1.0, 1.5, 0.5], "d": [5.0, 6.0, 4.0]}
    clock = Clock({k: [sizing[k]] + v for k, v in scripted.items()}, log)
    out = rate_kit.alternate({k: form(k, log) for k in sizing}, 3, clock=clock)
    want_iters = {"a": 50, "b": 33, "c": 2, "d": 2}
    # every form is warmed up (one call, then a sizing clock call of 2) before any repeat
    assert log[:8] == [e for k in "abcd" for e in (("call", k), ("clock", k, 2))]
    # then strict turns, `repeats` times each, at the sized iteration counts
    assert log[8:] == [("clock", k, want_iters[k]) for _ in range(3) for k in "abcd"]
    assert out == {k: sorted(v) for k, v in scripted.items()}
    assert list(out) == list("abcd")


def test_alternate_runs_a_setup_once_per_repeat_in_front_of_the_clock():
    log = []
    clock = Clock({"plain": [1.0] * 4, "switched": [1.0] * 4}, log)
    forms = {"plain": form("plain", log), "switched": (lambda: log.append(("setup",)), form("switched", log))}
    rate_kit.alternate(forms, 3, clock=clock)
    assert log.count(("setup",)) == 1 + 3                       # the warm-up and every repeat
    for i, e in enumerate(log):
        if e == ("setup",):                                     # next comes this form's call or clock call, never its neighbour's
            assert log[i + 1] in (("call", "switched"), ("clock", "switched", 50))
    repeats = log[4 + 1:]                                       # behind plain's two and switched's three warm-up entries
    assert repeats == [("clock", "plain", 50), ("setup",), ("clock", "switched", 50)] * 3


def test_show_prints_the_row_and_returns_the_median(capsys):
    assert rate_kit.show("a row", 2000, [1.0, 2.0, 4.0], base=1.0, against="its base") == 2.0
    line = capsys.readouterr().out
    for part in ("[1.000 .. 4.000]", "spread 3.000 ms", "1.00 M/s", "+100.00 % against its base"):
        assert part in line, (part, line)
    rate_kit.show("a row", 2000, [1.0, 2.0, 4.0])
    assert "against" not in capsys.readouterr().out


def test_cli():
    assert rate_kit.cli([]) == (5, 20, None, [])
    assert rate_kit.cli(["7", "18", "--parent", "x.so", "--only-small"]) == (7, 18, "x.so", ["--only-small"])
    assert rate_kit.cli(["unchanged", "4"]) == (4, 20, None, ["unchanged"])
    assert rate_kit.cli(["5", "20", "baseline"]) == (5, 20, None, ["baseline"])
    with pytest.raises(AssertionError):
        rate_kit.cli(["2"])


def test_parent_ab_alternates_builds_and_attributes_markers(tmp_path):
    order = tmp_path / "order.txt"
    child = tmp_path / "child.py"
    child.write_text(textwrap.dedent(f"""
        import os, sys
        lib = os.environ["EDDSA_AMD_LIBRARY"]
        with open({str(order)!r}, "a") as f:
            f.write(lib + " " + " ".join(sys.argv[1:]) + "\\n")
        turn = sum(1 for l in open({str(order)!r}) if l.startswith(lib))
        base = 10.0 if lib == "parent.so" else 20.0
        print("some other line")
        print("KEYED 1.0 (a line of the child's own: not a result)")
        print("RATE_KIT_CHILD UNKEYED", base + 3 - turn, base + 0.5)
        print("RATE_KIT_CHILD KEYED", 2 * base + turn)
    """))
    rows = rate_kit.parent_ab(str(child), 14, 2, "--child", ("UNKEYED", "KEYED"), "parent.so", "mine.so")
    assert order.read_text().splitlines() == [f"{lib} 3 14 --child" for lib in ("parent.so", "mine.so", "parent.so", "mine.so")]
    assert rows == {("parent", "UNKEYED"): [10.5, 10.5, 11.0, 12.0], ("parent", "KEYED"): [21.0, 22.0],
                    ("this", "UNKEYED"): [20.5, 20.5, 21.0, 22.0], ("this", "KEYED"): [41.0, 42.0]}


def test_importing_the_kit_loads_neither_the_library_nor_the_device():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import rate_kit; "
            "assert 'libeddsa_amd' not in sys.modules and 'torch' not in sys.modules; print('clean')")
    out = subprocess.check_output([sys.executable, "-c", code, rate_kit.ROOT + "/tools"], text=True)
    assert out.strip() == "clean"
