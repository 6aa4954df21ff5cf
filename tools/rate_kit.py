"""The measuring method of the rate scripts under tools/, once: the clocks, the alternation of forms in one process, the alternation
of two builds in fresh processes, the line a row is printed as, and the preamble that finds the tree and binds the library.

The rule the scripts share: forms that are compared run in the SAME call, taking turns, and every row shows its median with
min .. max and the spread, so that a difference can be read against the noise of the run it was measured in.

Importing this module loads neither torch's device side nor the library: only bind() and the clocks do.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIBRARY = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_debug.so")
CHILD_FLAG = "--only-unchanged"                     # what parent_ab's child processes are started with (internal)
CHILD_LINE = "RATE_KIT_CHILD"                       # what a line of a child's results begins with (emit, parent_ab)
LABEL_WIDTH = 58


def bind(debug=True):
    """The tree's libeddsa_amd, initialised on device 0.  debug: the debug build (the product's objects plus the hooks: route
    selection, phase timings, traces) unless EDDSA_AMD_LIBRARY names a library, which is then bound as given.  A script that uses
    torch imports it before it binds: the library shares torch's HIP runtime (api.py), and bound the other way round a script
    was seen to take twice as long to start."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import libeddsa_amd as ed
    if debug and not os.environ.get("EDDSA_AMD_LIBRARY"):
        ed.use_debug_library()
    ed.init(0)
    return ed


def timed(fn, iters):
    """ms per call: `iters` calls between two device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                            # untimed: the repeat starts from this form's own state, not from its neighbour's
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def wall(fn, iters=1):
    """ms per call on the host's clock, the device idle at both ends"""
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def steady(fn, warm=5, iters=30):
    """ms per call of back-to-back calls (no host wait between them) on the host's clock, after `warm` untimed ones"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def _synchronize():
    """alternate()'s wait behind a warm-up call - but only where torch's device side is up.  A caller that drives the library with
    host buffers alone and never initialised it gets NO wait here: such a script synchronises in its forms or in its clock (wall)."""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        torch.cuda.synchronize()


def alternate(forms, repeats, clock=timed):
    """forms: {label: callable or (setup, callable)} -> {label: sorted per-call ms of `repeats` repeats}, the forms taking turns.
    A set-up (a process-wide switch, say) runs once per repeat in front of its form's clock call, outside the timed window."""
    forms = {k: f if isinstance(f, tuple) else (None, f) for k, f in forms.items()}
    iters = {}
    for k, (setup, fn) in forms.items():            # warm-up; sizes a repeat to about 0.1 s
        if setup:
            setup()
        fn(); _synchronize()
        iters[k] = max(2, min(50, int(100.0 / max(clock(fn, 2), 1e-3))))
    out = {k: [] for k in forms}
    for _ in range(repeats):
        for k, (setup, fn) in forms.items():
            if setup:
                setup()
            out[k].append(clock(fn, iters[k]))
    return {k: sorted(v) for k, v in out.items()}


def show(label, n, ms, base=None, against=""):
    """one row: median, min .. max, spread, rate, and the median against `base`; returns the median"""
    med = ms[len(ms) // 2]
    rel = "" if base is None else f"  {100 * (med - base) / base:+6.2f} % against {against}"
    print(f"  {label:{LABEL_WIDTH}s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


def phase_split(forms):
    """the per-kernel split of every form: ten calls under the phase timer (verify_phase_ms: prepare, main, finish)"""
    import torch
    import libeddsa_amd as ed
    print("  per kernel (ms): prepare (+ tables, halve) / main / finish")
    for k, fn in forms.items():
        ed.set_profiling(True)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ph = ed.verify_phase_ms()
        ed.set_profiling(False)
        print(f"    {k:8s} {ph[0]:.3f} / {ph[1]:.3f} / {ph[2]:.3f}")


def rnd(seed):
    """rnd(seed)(*shape): uniform bytes on the device, all from one seeded generator"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)


def keyed_items(n, nkeys, sk_all, pk_all, msg):
    """n signed items with their keys drawn from the first nkeys: item i under key (i * 2654435761) mod nkeys -> sig, pk, idx"""
    import torch
    import libeddsa_amd as ed
    who = (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761) % nkeys
    sk, pk = sk_all[who].contiguous(), pk_all[who].contiguous()
    sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
    return sig, pk, who.to(torch.int32).contiguous()


def cli(argv):
    """[repeats=5] [log2 n=20] [--parent LIB] and whatever else -> repeats, log2 n, LIB or None, the other arguments in order"""
    argv, parent, numbers, flags = list(argv), None, [], []
    while argv:
        a = argv.pop(0)
        if a == "--parent":
            parent = argv.pop(0)
        elif a.isdigit() and len(numbers) < 2:
            numbers.append(a)
        else:
            flags.append(a)
    repeats = int(numbers[0]) if len(numbers) > 0 else 5
    log_n = int(numbers[1]) if len(numbers) > 1 else 20
    assert repeats >= 3
    return repeats, log_n, parent, flags


def emit(results):
    """a child of parent_ab hands its results back: one line per marker, `RATE_KIT_CHILD MARKER ms ms ..`"""
    for marker, ms in results.items():
        print(CHILD_LINE, marker, " ".join(f"{x:.4f}" for x in ms), flush=True)


def parent_ab(script, log_n, repeats, child_flag, markers, parent, mine):
    """Two builds of the library against each other: `script 3 log_n child_flag` in fresh processes, one after another, parent and
    this build alternating `repeats` times, the library handed over in EDDSA_AMD_LIBRARY.  Every child prints one line per marker
    with emit(); whatever else it prints is ignored -> {(build, marker): sorted ms}, build in ("parent", "this")."""
    rows = {(build, m): [] for build in ("parent", "this") for m in markers}
    for _ in range(repeats):
        for build, lib in (("parent", parent), ("this", mine)):
            out = subprocess.check_output([sys.executable, os.path.abspath(script), "3", str(log_n), child_flag],
                                          env=dict(os.environ, EDDSA_AMD_LIBRARY=lib), text=True, timeout=300)
            lines = {l.split()[1]: l.split()[2:] for l in out.splitlines() if l.startswith(CHILD_LINE + " ")}
            for m in markers:
                rows[(build, m)] += [float(x) for x in lines[m]]
    return {k: sorted(v) for k, v in rows.items()}
