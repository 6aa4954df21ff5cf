"""ctypes binding of libeddsa_amd.so.

Batch functions accept either
  * torch CUDA tensors (dtype uint8, contiguous): the device-pointer entry points are used,
    work is enqueued on torch's current stream and the result tensor is returned without a
    host synchronisation; or
  * numpy uint8 arrays / bytes: the host-pointer entry points are used (copy in, run, copy out).
Item layout is the packed item-major layout of include/eddsa_amd.h.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_c_size = ctypes.c_size_t
_c_ptr = ctypes.c_void_p


class EddsaAmdError(RuntimeError):
    """A HIP call behind the engine failed (or the engine library is missing)."""


_PATH = None


def library_path():
    """The in-tree product build, libeddsa_amd.so - unless use_debug_library() chose the debug build, or EDDSA_AMD_LIBRARY
    names another build of the same sources (tools/ab.sh: A/B measurements load their variants this way and never
    overwrite the product library)."""
    return os.environ.get("EDDSA_AMD_LIBRARY") or _PATH or os.path.join(_HERE, "libeddsa_amd.so")


def use_debug_library():
    """Bind libeddsa_amd_debug.so instead: the product's object files plus the test and measurement hooks of
    include/eddsa_amd_debug.h (route selection, phase timings, fault injectors, traces), which the shipped library does not
    export.  The tests, bench.py and the scripts under tools/ call this before their first call; a process holds ONE engine
    library, so it must come before anything has loaded the product build."""
    global _PATH
    path = os.path.join(_HERE, "libeddsa_amd_debug.so")
    if _LIB is not None and library_path() != path:
        raise EddsaAmdError(f"use_debug_library(): {library_path()} is already loaded in this process")
    _PATH = path


def _share_the_hip_runtime_with_torch():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's,
    which libeddsa_amd.so is linked against); whichever is loaded first serves both.  If this library came first,
    a later `import torch` would bring a second runtime, and the first one then finds no device.  So when PyTorch is
    installed but not yet imported, load its runtime before ours - the one its tensors will live in."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for d in (spec.submodule_search_locations or []) if spec else []:
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(d, "lib", name)
            if os.path.exists(path):
                try:
                    ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
                except OSError:
                    return


def library():
    """Load libeddsa_amd.so (built in-tree by `make` / __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise EddsaAmdError(
                f"{path} is missing: build it with `make` (hipcc --offload-arch=gfx950); "
                "there is no CPU fallback")
        _share_the_hip_runtime_with_torch()
        lib = ctypes.CDLL(path)
        global _PATH
        _PATH = _PATH or path                                          # (what is loaded stays loaded)
        lib.eddsa_amd_strerror.restype = ctypes.c_char_p
        lib.ed25519_verify.restype = ctypes.c_bool
        lib.eddsa_verify.restype = ctypes.c_bool
        _LIB = lib
    return _LIB


def _check(rc, what):
    if rc != 0:
        msg = library().eddsa_amd_strerror(rc).decode()
        raise EddsaAmdError(f"{what}: {msg} (rc={rc}); the engine has no CPU fallback")


def init(device=None):
    """Bind the engine to a HIP device (default: torch's / HIP's current device)."""
    if device is None:
        try:
            import torch
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        except ImportError:
            device = 0
    _check(library().eddsa_amd_init(int(device)), "eddsa_amd_init")


def shutdown():
    """release every device resource of the engine; the next call initialises it again (and disarms the test hooks)"""
    library().eddsa_amd_shutdown()


# ---------------------------------------------------------------------------------------------
# the test and measurement surface (include/eddsa_amd_debug.h); not part of the product contract
# ---------------------------------------------------------------------------------------------

HOOKS_OFF = -100002
LAYER_OPS = {"fe_mul": 1, "fe_sq": 2, "fe_inv": 3, "fe_pow2523": 4, "fe_mul_loose": 5, "sc_reduce32": 6, "sc_reduce64": 7,
             "sc_muladd": 8, "sha512": 9, "ed_import_export": 10, "ed_scale_base": 11, "ed_dual_scale": 12, "ge_dbl_add": 13,
             "x25519_ladder": 14}


def _hooks():
    """the loaded library, which must be the debug build (use_debug_library): the shipped one exports no hook"""
    lib = library()
    if not hasattr(lib, "eddsa_amd_debug_init"):
        raise EddsaAmdError(f"{library_path()} has no test hooks: call libeddsa_amd.use_debug_library() before the first "
                            "call (or point EDDSA_AMD_LIBRARY at libeddsa_amd_debug.so)")
    return lib


def debug_init(device=0, hooks=True):
    """eddsa_amd_init(device), then arm (or disarm) the fault injectors"""
    _check(_hooks().eddsa_amd_debug_init(int(device), ctypes.c_uint(1 if hooks else 0)), "eddsa_amd_debug_init")


def debug_fail_next_host_call():
    """the next host-pointer call fails after its kernels were launched; returns HOOKS_OFF when the hooks are not armed"""
    return int(_hooks().eddsa_amd_debug_fail_next_host_call())


def debug_fail_hip_call(nth):
    """the nth checked HIP call of the verify passes from now on fails (0 disarms); HOOKS_OFF when not armed"""
    return int(_hooks().eddsa_amd_debug_fail_hip_call(int(nth)))


def debug_hip_calls():
    return int(_hooks().eddsa_amd_debug_hip_calls())


STALLED = -100003


def debug_withhold_handoff(tile_plus_1):
    """the first hand-off of that tile of k_verify_exact_lane_chain is never published, and the flag of that window point of
    group 0 of the batch verification never raised, in the passes that follow (0: off); HOOKS_OFF when not armed, otherwise
    the number of Horner waves of the batch verification that gave up since the previous call"""
    return int(_hooks().eddsa_amd_debug_withhold_handoff(int(tile_plus_1)))


def debug_teardown_errors():
    """(count, first hipError_t) of the HIP calls that failed on teardown / clean-up paths since the library was loaded"""
    first = ctypes.c_int(0)
    return int(_hooks().eddsa_amd_debug_teardown_errors(ctypes.byref(first))), int(first.value)


_PROBE = None


def probe_library():
    """libeddsa_amd_probe.so (include/eddsa_amd_probe.h): the layer probes, test infrastructure built from the same device
    source as the product's kernels and loaded BESIDE the product - libeddsa_amd.so holds none of its kernels."""
    global _PROBE
    if _PROBE is None:
        path = os.path.join(_HERE, "libeddsa_amd_probe.so")
        if not os.path.exists(path):
            raise EddsaAmdError(f"{path} is missing: build it with `make probe`")
        library()                                  # (the one HIP runtime of the process is settled there)
        _PROBE = ctypes.CDLL(path)
    return _PROBE


def debug_layer(op, items, out_w, form=0):
    """run one layer of the device code (include/eddsa_amd_probe.h) on `items` (equal-length byte strings): -> list of
    out_w-byte results.  Runs on the current HIP device through the probe library."""
    code = LAYER_OPS[op] if isinstance(op, str) else int(op)
    n = len(items)
    in_w = len(items[0]) if n else 32
    assert all(len(x) == in_w for x in items)
    buf = np.frombuffer(b"".join(items), np.uint8).copy() if n else np.zeros(1, np.uint8)
    out = np.zeros(max(n, 1) * out_w, np.uint8)
    _check(probe_library().eddsa_amd_probe_layer(ctypes.c_int(code), ctypes.c_int(form), _np_ptr(out), _c_size(out_w), _np_ptr(buf),
                                                 _c_size(in_w), _c_size(n)), f"eddsa_amd_probe_layer({op})")
    return [out[out_w * i:out_w * (i + 1)].tobytes() for i in range(n)]


def verify_phase_ms():
    """(prepare, main, finish) kernel durations in ms of the last profiled verify pass, measured
    with HIP events on the launch stream (enable with set_profiling(True))."""
    out = (ctypes.c_float * 3)()
    _check(_hooks().eddsa_amd_verify_phase_ms(out), "eddsa_amd_verify_phase_ms")
    return tuple(out)


# the opt-in strict rules of verification: include/eddsa_amd.h, EDDSA_AMD_VERIFY_*
VERIFY_S_BELOW_L = 0x100
VERIFY_A_CANONICAL = 0x200
VERIFY_A_NOT_SMALL = 0x400
VERIFY_R_NOT_SMALL = 0x800
VERIFY_STRICT = 0xF00
_VERIFY_POLICY_MASK = 0xF00
# the two halves of the word eddsa_amd_set_offcurve_mode takes: each setter remembers its own and sends both
_offcurve_mode = 1
_verify_policy = 0


def _send_mode_word():
    library().eddsa_amd_set_offcurve_mode(_offcurve_mode | _verify_policy)


def set_offcurve_mode(exact=True):
    """exact=True (default): off-curve public keys are verified in the reference's own operation
    order; False: they are rejected outright (differs only on a SHA-512 fixed point); 2: every item
    takes the reference-order path (self-check mode, slow).  The verify policy (set_verify_policy) stays as it is."""
    global _offcurve_mode
    _offcurve_mode = 2 if exact == 2 else int(bool(exact))
    _send_mode_word()


def set_verify_policy(policy=0):
    """the opt-in strict rules every form of verification applies from now on, process-wide: an OR of VERIFY_S_BELOW_L (S < l),
    VERIFY_A_CANONICAL (the key is an encoding RFC 8032 5.1.3 decodes), VERIFY_A_NOT_SMALL / VERIFY_R_NOT_SMALL (no key / R of
    order 1, 2, 4 or 8); VERIFY_STRICT = all four; 0 (default) = the reference's verdicts.  A policy only turns accepts into
    rejects.  ValueError for any other bit; the off-curve mode (set_offcurve_mode) stays as it is."""
    global _verify_policy
    policy = int(policy)
    if policy & ~_VERIFY_POLICY_MASK:
        raise ValueError(f"set_verify_policy: {policy:#x} has bits outside VERIFY_STRICT ({_VERIFY_POLICY_MASK:#x})")
    _verify_policy = policy
    _send_mode_word()


# the equation an item is held to: include/eddsa_amd.h, EDDSA_AMD_EQUATION_*
EQUATION_COFACTORLESS = 0
EQUATION_COFACTORED = 1


def set_verify_equation(cofactored=False):
    """the equation every form of verification holds an item to from now on, process-wide: False / EQUATION_COFACTORLESS
    (default) = the reference's check, True / EQUATION_COFACTORED = the rules of ZIP-215: S < l, A and R any encoding that
    decodes, [8](S B - t A - R) = 0 - the rule under which single and batch verification always agree.  A call of its own:
    the off-curve mode (set_offcurve_mode) and the verify policy (set_verify_policy) stay as they are."""
    _check(library().eddsa_amd_set_verify_equation(ctypes.c_int(int(cofactored))), "eddsa_amd_set_verify_equation")


def set_verify_algo(algo=0):
    """0 (default): half-length scalars (four lanes per item up to 24 576 items, one above); 1: always full-length;
    2: half-length with one lane per item whatever the size; 3: the arrangement of 24 577 .. 2^18 items (three-lane
    preparation, one-lane evaluation) at any size below 2^18; 4: the arrangement of full-size passes (balanced pairs, 33 windows)
    at any size.  Same verdicts; a measurement and test aid."""
    _hooks().eddsa_amd_set_verify_algo(int(algo))


def debug_halve(ts, wide=False):
    """diagnostic: the device's pair search on scalars t (ints below l); returns a list of (found, u, v).  wide: False = pairs
    below 2^134, True = below 2^138, 2 = the balanced search of full-size passes (both up to B33, 33 windows)"""
    n = len(ts)
    tin = np.frombuffer(b"".join(int(t).to_bytes(32, "little") for t in ts), np.uint8).copy()
    out = np.zeros(48 * max(n, 1), np.uint8)
    _check(probe_library().eddsa_amd_probe_halve(out.ctypes.data_as(ctypes.c_void_p), tin.ctypes.data_as(ctypes.c_void_p), _c_size(n),
                                                 ctypes.c_int(2 if wide == 2 and wide is not True else int(bool(wide)))), "eddsa_amd_probe_halve")
    res = []
    for i in range(n):
        row = out[48 * i:48 * i + 48].tobytes()
        u = int.from_bytes(row[20:40], "little") * (-1 if row[40] else 1)
        res.append((bool(row[41]), u, int.from_bytes(row[:20], "little")))
    return res


def halve_rejected():
    """diagnostic: half-length pairs refused by the exact integer check on the default device (expected 0)"""
    out = ctypes.c_uint64(0)
    _check(_hooks().eddsa_amd_halve_rejected(ctypes.byref(out)), "eddsa_amd_halve_rejected")
    return int(out.value)


# region -> (its number in include/eddsa_amd_debug.h, dtype, bytes per item, bytes per group, the shape of one item's / group's part)
_RLC_REGIONS = {"info": (0, np.uint64, 0, 0, ()), "leaf": (1, np.uint8, 32, 0, (32,)), "seed": (2, np.uint8, 0, 0, ()),
                "ts": (3, np.uint8, 64, 0, (2, 32)), "flags": (4, np.uint8, 1, 0, ()), "dig": (5, np.int8, 0, 48 * 8192, (48, 8192)),
                "bdig": (6, np.int8, 0, 32, (32,)), "gflags": (7, np.uint32, 0, 4, ()), "gok": (8, np.uint8, 0, 1, ()),
                "seg": (9, np.uint8, 0, 48 * 128, (48, 4, 32))}


def debug_rlc_snapshot(region):
    """diagnostic: one region of what the last pass of the batch verification on the default device left in its workspace
    (eddsa_amd_debug_rlc_snapshot; waits for the device, reads only), trimmed to the pass's n items and its groups: "info" -> (n,
    groups, capacity); "seed" -> 32 bytes; "leaf" (n, 32) uint8; "ts" (n, 2, 32) uint8, t mod l and S mod l little-endian; "flags"
    (n,) uint8; "dig" (groups, 48, 8192) int8, rows 0..31 the keys' digits and 32..47 those of z; "bdig" (groups, 32) int8;
    "gflags" (groups,) uint32; "gok" (groups,) uint8; "seg" (groups, 48, 4, 32) uint8, the packed window points
    Y-X | Y+X | 2dT | 2Z.  EddsaAmdError when no such pass has run."""
    lib = _hooks()
    code, dtype, per_item, per_group, shape = _RLC_REGIONS[region]
    info = np.zeros(3, np.uint64)
    _check(min(lib.eddsa_amd_debug_rlc_snapshot(ctypes.c_int(0), _np_ptr(info), _c_size(info.nbytes)), 0), "eddsa_amd_debug_rlc_snapshot")
    n, groups = int(info[0]), int(info[1])
    if region == "info":
        return n, groups, int(info[2])
    nbytes = 32 if region == "seed" else n * per_item + groups * per_group
    out = np.zeros(nbytes, np.uint8)
    got = lib.eddsa_amd_debug_rlc_snapshot(ctypes.c_int(code), _np_ptr(out), _c_size(nbytes))
    _check(min(got, 0), "eddsa_amd_debug_rlc_snapshot")
    if got != nbytes:
        raise EddsaAmdError(f"eddsa_amd_debug_rlc_snapshot({region}): {got} bytes, expected {nbytes}")
    if region == "seed":
        return out.tobytes()
    return out.view(dtype).reshape((n if per_item else groups,) + shape)


RLC_MIN_ITEMS_DEFAULT = 5 << 15                # EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT, include/eddsa_amd.h


def set_rlc_min_items(items):
    """ed25519_verify_batch_rlc calls with fewer items go straight to the per-item kernels (default 5 x 2^15 = 163 840: above the
    measured break-even of about 2^17 items; 0 = always try the combination)"""
    library().eddsa_amd_set_rlc_min_items(_c_size(int(items)))


def set_host_threads(n):
    """helper threads that stage ordinary host memory into the pipeline's page-locked buffers (default 6, 0..16)"""
    library().eddsa_amd_set_host_threads(int(n))


def combiner_stats():
    """(launches, calls they carried) of the combiner of small host-pointer calls on the default device"""
    out = (ctypes.c_uint64 * 2)()
    _check(_hooks().eddsa_amd_combiner_stats(out), "eddsa_amd_combiner_stats")
    return int(out[0]), int(out[1])


_PINNED = {}


def host_array(shape, dtype=np.uint8):
    """a numpy array in page-locked host memory (eddsa_amd_host_alloc): the host-pointer entry points read and
    write such arrays in place, without a staging copy.  Release it with host_free()."""
    lib = library()
    lib.eddsa_amd_host_alloc.restype = ctypes.c_void_p
    count = int(np.prod(shape))
    nbytes = max(count * np.dtype(dtype).itemsize, 1)
    ptr = lib.eddsa_amd_host_alloc(_c_size(nbytes))
    if not ptr:
        raise EddsaAmdError("eddsa_amd_host_alloc failed")
    buf = (ctypes.c_uint8 * nbytes).from_address(ptr)
    _PINNED[ptr] = buf
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def host_free(a):
    """release an array made by host_array (the array must not be used afterwards)"""
    ptr = a.ctypes.data
    if _PINNED.pop(ptr, None) is not None:
        library().eddsa_amd_host_free(_c_ptr(ptr))


def set_profiling(on):
    _hooks().eddsa_amd_set_profiling(int(bool(on)))


def secret_residue():
    """(aux, acc, staging-in, staging-out): non-zero bytes left in the engine's secret-bearing HBM
    buffers on the default device (diagnostic for the hygiene tests; waits for the device)."""
    out = (ctypes.c_uint64 * 4)()
    _check(_hooks().eddsa_amd_secret_residue(out), "eddsa_amd_secret_residue")
    return tuple(int(x) for x in out)


def init_devices(devices=None):
    """Bind the device set of the *_multi entry points (default: every visible device): one engine and
    one RCCL communicator per device, single process."""
    if devices is None:
        _check(library().eddsa_amd_init_devices(None, 0), "eddsa_amd_init_devices")
    else:
        arr = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        _check(library().eddsa_amd_init_devices(arr, len(devices)), "eddsa_amd_init_devices")
    return int(library().eddsa_amd_device_count())


def device_count():
    return int(library().eddsa_amd_device_count())


# ---------------------------------------------------------------------------------------------
# argument plumbing
# ---------------------------------------------------------------------------------------------

def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _as_np(x, width, name):
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.asarray(x)
    if a.dtype != np.uint8:
        raise TypeError(f"{name}: expected uint8 data")
    a = np.ascontiguousarray(a)
    if width and a.size % width:
        raise ValueError(f"{name}: size {a.size} is not a multiple of {width}")
    return a


def _np_ptr(a):
    return a.ctypes.data_as(_c_ptr)


def _torch_check(t, width, name):
    import torch
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous CUDA uint8 tensor")
    if width and t.numel() % width:
        raise ValueError(f"{name}: size {t.numel()} is not a multiple of {width}")
    return t


def _stream():
    import torch
    return _c_ptr(torch.cuda.current_stream().cuda_stream)


def _msg_span(total, msg_off, msg_len, n, on_device):
    """how `total` message bytes are cut into n messages -> (the offset table or None, msg_len): msg_len bytes each (default
    total / n), or ragged by msg_off[0..n] - on the device n+1 64-bit words (the kernels read them as uint64)"""
    if msg_off is None:
        if msg_len is None:
            if n and total % n:
                raise ValueError("msgs: size is not a multiple of the batch size; pass msg_len or msg_off")
            msg_len = total // n if n else 0
        return None, int(msg_len)
    if on_device:
        import torch
        if not _is_torch(msg_off) or not msg_off.is_cuda or not msg_off.is_contiguous() or \
                msg_off.dtype not in (torch.int64, torch.uint64) or msg_off.numel() != n + 1:
            raise ValueError("msg_off: expected n+1 contiguous int64/uint64 offsets on the device")
        return msg_off, 0
    off = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
    if off.size != n + 1 or (n and int(off[-1]) > total):
        raise ValueError("msg_off: expected n+1 offsets within msgs")
    return off, 0


def _run_32(fn_host, fn_dev, what, inputs, out_width, n_from):
    """common driver for fixed-width kernels: inputs = [(array, width, name), ...]"""
    lib = library()
    first = inputs[0][0]
    if _is_torch(first):
        import torch
        ts = [_torch_check(t, w, nm) for t, w, nm in inputs]
        n = ts[0].numel() // n_from
        for t, (_, w, nm) in zip(ts, inputs):
            if t.numel() // w != n:
                raise ValueError(f"{what}: {nm} holds {t.numel() // w} items, expected {n}")
        out = torch.empty((n, out_width), dtype=torch.uint8, device=ts[0].device)
        args = [_c_ptr(out.data_ptr())] + [_c_ptr(t.data_ptr()) for t in ts] + [_c_size(n), _stream()]
        _check(getattr(lib, fn_dev)(*args), what)
        return out
    arrs = [_as_np(a, w, nm) for a, w, nm in inputs]
    n = arrs[0].size // n_from
    for a, (_, w, nm) in zip(arrs, inputs):
        if a.size // w != n:
            raise ValueError(f"{what}: {nm} holds {a.size // w} items, expected {n}")
    out = np.zeros((n, out_width), dtype=np.uint8)
    args = [_np_ptr(out)] + [_np_ptr(a) for a in arrs] + [_c_size(n)]
    _check(getattr(lib, fn_host)(*args), what)
    return out


def _key_indices(name, key_idx, n, on_device):
    """the key indices of a keyed call, uint32 on the host and int32 (read as unsigned) on the device -> (the array, its length);
    n None: the array sets the batch size, else it must hold n indices"""
    if on_device:
        import torch
        if not _is_torch(key_idx) or key_idx.dtype != torch.int32 or not key_idx.is_cuda or not key_idx.is_contiguous():
            raise ValueError(f"{name}: key_idx: expected contiguous int32 indices on the device")
        count = key_idx.numel()
    else:
        key_idx = np.ascontiguousarray(np.asarray(key_idx))
        if key_idx.dtype != np.uint32:
            raise ValueError(f"{name}: key_idx: expected uint32 indices")
        count = key_idx.size
    if n is not None and count != n:
        raise ValueError(f"{name}: key_idx holds {count} indices, expected {n}")
    return key_idx, count


def _run_items(name, lead, data, out_shape, keyed=None, fixed=None, data_name="msgs", msg_off=None, msg_len=None, context=None,
               stats=None, dev=True, sizes_first=False):
    """The one driver of the calls that carry items and messages -> (n,) + out_shape uint8.  numpy / bytes: the host form `name`;
    CUDA tensors (dev false: host pointers only): `name`_dev on torch's stream.  The C argument list is
        out [, stats] [, handle, key_idx] , lead arrays... , data [, msg_off, msg_len] , n [, context, context_len] [, stream]
    lead     the fixed-width arrays [(array, bytes per item, name), ...] in the C order
    keyed    (Keyset or Signer, key_idx) of a keyed call; without a lead array key_idx sets the batch size
    data     ragged / fixed-length messages (msg_off, msg_len), or `fixed` bytes per item under the name data_name (digests,
             prehashes), which the C function takes without offsets and length
    context  None: the C function takes none; else what _context() made of the caller's
    stats    None: the C function takes no statistics; true -> (output, the four counters); false on the device: NULL is
             passed, nothing is counted
    sizes_first  the batch sizes are compared before `data` is looked at (which complaint a doubly wrong call gets)"""
    ctx_args = [] if context is None else [ctypes.c_char_p(context), _c_size(len(context))]
    handle = [keyed[0]._handle()] if keyed else []
    on_device = dev and _is_torch(lead[0][0] if lead else keyed[1])
    check, size, ptr = (_torch_check, lambda t: t.numel(), lambda t: _c_ptr(t.data_ptr())) if on_device else \
                       (_as_np, lambda a: a.size, _np_ptr)
    arrs = [check(a, w, nm) for a, w, nm in lead]
    if not sizes_first:
        data = check(data, fixed or 0, data_name)
    n = size(arrs[0]) // lead[0][1] if lead else None
    for a, (_, w, nm) in zip(arrs[1:], lead[1:]):
        if size(a) // w != n:
            raise ValueError(f"{name}: {lead[0][2]} and {nm} disagree on the batch size")
    if keyed:
        key_idx, n = _key_indices(name, keyed[1], n, on_device)
        arrs.insert(0, key_idx)
    if sizes_first:
        data = check(data, fixed or 0, data_name)
    if fixed:
        if size(data) != fixed * n:
            raise ValueError(f"{name}: {data_name} holds {size(data) // fixed} items of {fixed} bytes, expected {n}")
        msg_args = []
    else:
        off, mlen = _msg_span(size(data), msg_off, msg_len, n, on_device)
        msg_args = [ptr(off) if off is not None else None, _c_size(mlen)]
    if on_device:
        import torch
        out = torch.empty((n,) + out_shape, dtype=torch.uint8, device=arrs[0].device)
        counts = torch.zeros((4,), dtype=torch.int32, device=arrs[0].device) if stats else None
    else:
        out = np.zeros((n,) + out_shape, dtype=np.uint8)
        counts = np.zeros(4, dtype=np.uint32)
    stats_args = [] if stats is None else [ptr(counts) if counts is not None else None]
    fn = getattr(library(), name + "_dev" if on_device else name)
    _check(fn(ptr(out), *stats_args, *handle, *[ptr(a) for a in arrs], ptr(data), *msg_args, _c_size(n), *ctx_args,
              *([_stream()] if on_device else [])), name)
    return (out, tuple(int(x) for x in (counts.cpu() if on_device else counts))) if stats else out


# ---------------------------------------------------------------------------------------------
# batched entry points (include/eddsa_amd.h)
# ---------------------------------------------------------------------------------------------

def x25519_batch(scalars, points):
    """loop of x25519 (reference lib/eddsa.h:67) -> (n, 32) uint8"""
    return _run_32("x25519_batch", "x25519_batch_dev", "x25519_batch",
                   [(scalars, 32, "scalars"), (points, 32, "points")], 32, 32)


def x25519_base_batch(scalars):
    """loop of x25519_base (reference lib/eddsa.h:64)"""
    return _run_32("x25519_base_batch", "x25519_base_batch_dev", "x25519_base_batch",
                   [(scalars, 32, "scalars")], 32, 32)


def ed25519_genpub_batch(secs):
    """loop of ed25519_genpub (reference lib/eddsa.h:44)"""
    return _run_32("ed25519_genpub_batch", "ed25519_genpub_batch_dev", "ed25519_genpub_batch",
                   [(secs, 32, "secs")], 32, 32)


def pk_ed25519_to_x25519_batch(pubs):
    """loop of pk_ed25519_to_x25519 (reference lib/eddsa.h:77)"""
    return _run_32("pk_ed25519_to_x25519_batch", "pk_ed25519_to_x25519_batch_dev",
                   "pk_ed25519_to_x25519_batch", [(pubs, 32, "pubs")], 32, 32)


def sk_ed25519_to_x25519_batch(secs):
    """loop of sk_ed25519_to_x25519 (reference lib/eddsa.h:80)"""
    return _run_32("sk_ed25519_to_x25519_batch", "sk_ed25519_to_x25519_batch_dev",
                   "sk_ed25519_to_x25519_batch", [(secs, 32, "secs")], 32, 32)


# the bits of a class byte: EDDSA_AMD_POINT_*, include/eddsa_amd.h
POINT_ON_CURVE = 0x01
POINT_CANONICAL = 0x02
POINT_SMALL_ORDER = 0x04
POINT_PRIME_SUBGROUP = 0x08


def point_classify_batch(points):
    """what each 32-byte string is as a curve point (include/eddsa_amd.h: ed25519_point_classify_batch) -> (n,) uint8, the OR of
    POINT_ON_CURVE, POINT_CANONICAL, POINT_SMALL_ORDER and POINT_PRIME_SUBGROUP; 0 for a string that is no curve point.  A key fit
    for registration has cls & 0x0F == POINT_ON_CURVE | POINT_CANONICAL | POINT_PRIME_SUBGROUP.  bytes / numpy: the host form;
    a CUDA uint8 tensor: the device form, on the current stream."""
    return _run_32("ed25519_point_classify_batch", "ed25519_point_classify_batch_dev", "ed25519_point_classify_batch",
                   [(points, 32, "points")], 1, 32).reshape(-1)


# what point_muladd_batch writes for a string that is no curve point: EDDSA_AMD_NO_POINT_BYTE0 and 31 zero bytes
NO_POINT = bytes([0x02]) + bytes(31)


def point_muladd_batch(points, mul=None, add=None, out=None):
    """[mul_i]points_i + [add_i]B as encoded points (include/eddsa_amd.h: ed25519_point_muladd_batch) -> (n, 32) uint8.  mul, add:
    32-byte little-endian integers in [0, 2^256), public derivation scalars - NOT secrets (the call is not constant-time); None:
    every mul_i = 1 / every add_i = 0.  A string that is no curve point gives NO_POINT.  bytes / numpy: the host form; CUDA uint8
    tensors: the device form, on the current stream.  out: None, or `points` itself for in-place derivation."""
    if out is not None and out is not points:
        raise ValueError("ed25519_point_muladd_batch: out must be None or points itself")
    lib = library()
    given = [(a, nm) for a, nm in ((points, "points"), (mul, "mul"), (add, "add")) if a is not None or nm == "points"]
    if _is_torch(points):
        import torch
        ts = {nm: _torch_check(a, 32, nm) for a, nm in given}
        n = ts["points"].numel() // 32
        for nm, t in ts.items():
            if t.numel() // 32 != n:
                raise ValueError(f"ed25519_point_muladd_batch: {nm} holds {t.numel() // 32} items, expected {n}")
        res = ts["points"] if out is not None else torch.empty((n, 32), dtype=torch.uint8, device=ts["points"].device)
        ptr = lambda nm: _c_ptr(ts[nm].data_ptr()) if nm in ts else None   # noqa: E731
        _check(lib.ed25519_point_muladd_batch_dev(_c_ptr(res.data_ptr()), ptr("points"), ptr("mul"), ptr("add"), _c_size(n), _stream()),
               "ed25519_point_muladd_batch_dev")
        return res.reshape(n, 32)
    arrs = {nm: _as_np(a, 32, nm) for a, nm in given}
    n = arrs["points"].size // 32
    for nm, a in arrs.items():
        if a.size // 32 != n:
            raise ValueError(f"ed25519_point_muladd_batch: {nm} holds {a.size // 32} items, expected {n}")
    if out is not None and (arrs["points"] is not points or not points.flags.writeable):
        raise ValueError("ed25519_point_muladd_batch: in place needs a writable contiguous uint8 array")
    res = arrs["points"] if out is not None else np.zeros((n, 32), dtype=np.uint8)
    ptr = lambda nm: _np_ptr(arrs[nm]) if nm in arrs else None   # noqa: E731
    _check(lib.ed25519_point_muladd_batch(_np_ptr(res), ptr("points"), ptr("mul"), ptr("add"), _c_size(n)), "ed25519_point_muladd_batch")
    return res.reshape(n, 32)


def ed25519_verify_batch(sigs, pubs, msgs, msg_off=None, msg_len=None):
    """loop of ed25519_verify (reference lib/eddsa.h:52) -> (n,) uint8, 1 = accept.

    msgs is the concatenation of all messages; either every message has msg_len bytes
    (default: len(msgs) / n) or msg_off[0..n] (uint64) gives the ragged boundaries."""
    return _run_items("ed25519_verify_batch", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], msgs, (), msg_off=msg_off, msg_len=msg_len)


def ed25519_verify_batch_rlc(sigs, pubs, msgs, msg_off=None, msg_len=None, return_stats=False):
    """OPT-IN batch verification by random linear combination (include/eddsa_amd.h: the reference's TODO,
    lib/ed25519-sha512.c:13-14): same arguments and verdicts as ed25519_verify_batch, groups that do not
    pass fall back to the per-item kernels.  return_stats=True -> (ok, (items decided by the combination,
    items decided per item, groups sent to the per-item kernels, groups decided by the combination))."""
    return _run_items("ed25519_verify_batch_rlc", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], msgs, (), msg_off=msg_off, msg_len=msg_len,
                      stats=bool(return_stats), sizes_first=True)


def ed25519_verify_digests(sigs, pubs, digests):
    """loop of ed25519_verify for callers that already hold digests[i] = SHA-512(R_i || A_i || M_i) (64 bytes per item, as
    hashlib.sha512(...).digest() returns them): no message is uploaded or hashed -> (n,) uint8, 1 = accept.  The caller vouches
    that each digest was computed over the R and A bytes of this call's sigs[i] and pubs[i] (include/eddsa_amd.h)."""
    return _run_items("ed25519_verify_digests", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], digests, (), fixed=64, data_name="digests")


def ed25519_verify_digests_rlc(sigs, pubs, digests, return_stats=False):
    """ed25519_verify_batch_rlc from caller-supplied digests (see ed25519_verify_digests): same verdicts, same statistics"""
    return _run_items("ed25519_verify_digests_rlc", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], digests, (), fixed=64, data_name="digests",
                      stats=bool(return_stats))


KEYSET_MAX_KEYS = 1 << 20                      # EDDSA_AMD_KEYSET_MAX_KEYS, include/eddsa_amd.h
KEYSET_COMB_MAX_KEYS = 1 << 14                 # EDDSA_AMD_KEYSET_COMB_MAX_KEYS: a comb key set holds 88 KiB of HBM per key


class Keyset:
    """A key set (include/eddsa_amd.h: eddsa_amd_keyset): public keys registered once, in HBM with their tables, for
    ed25519_verify_keyed.  Immutable; lives until close() (or the end of a `with` block), also across shutdown()."""

    def __init__(self, handle):
        self._h = handle

    def _handle(self):
        if self._h is None:
            raise ValueError("Keyset: already closed")
        return self._h

    @property
    def count(self):
        lib = library()
        lib.eddsa_amd_keyset_count.restype = ctypes.c_size_t
        return int(lib.eddsa_amd_keyset_count(self._handle()))

    @property
    def device(self):
        return int(library().eddsa_amd_keyset_device(self._handle()))

    @property
    def comb(self):
        """whether the set holds a comb per key (keyset_create(keys, comb=True)): keyed passes over it take the comb route"""
        return bool(library().eddsa_amd_keyset_is_comb(self._handle()))

    @property
    def nbytes(self):
        """the HBM the set holds"""
        lib = library()
        lib.eddsa_amd_keyset_bytes.restype = ctypes.c_size_t
        return int(lib.eddsa_amd_keyset_bytes(self._handle()))

    def classify(self):
        """the class byte of every key of the set (point_classify_batch over the set's own bytes in HBM) -> (count,) uint8, host"""
        cls = np.zeros(self.count, dtype=np.uint8)
        _check(library().eddsa_amd_keyset_classify(self._handle(), _np_ptr(cls)), "eddsa_amd_keyset_classify")
        return cls

    def close(self):
        if self._h is not None:
            library().eddsa_amd_keyset_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def keyset_create(keys, comb=False):
    """keys: count x 32 bytes, numpy / bytes (host form, on the default device) or a CUDA uint8 tensor (on its device) -> Keyset.
    Any 32-byte strings may be registered; returns once the tables are built.  comb=True: a comb key set (at most
    KEYSET_COMB_MAX_KEYS keys, 88 KiB of HBM per key on top) - the same verdicts from 88 additions and 6 doublings per item."""
    lib = library()
    h = _c_ptr()
    suffix = "_comb" if comb else ""
    if _is_torch(keys):
        keys = _torch_check(keys, 32, "keys")
        fn = getattr(lib, "eddsa_amd_keyset_create" + suffix + "_dev")
        _check(fn(ctypes.byref(h), _c_ptr(keys.data_ptr()), _c_size(keys.numel() // 32), _stream()), "eddsa_amd_keyset_create" + suffix + "_dev")
    else:
        keys = _as_np(keys, 32, "keys")
        fn = getattr(lib, "eddsa_amd_keyset_create" + suffix)
        _check(fn(ctypes.byref(h), _np_ptr(keys), _c_size(keys.size // 32)), "eddsa_amd_keyset_create" + suffix)
    return Keyset(h)


def ed25519_verify_keyed(sigs, keyset, key_idx, msgs, msg_off=None, msg_len=None):
    """ed25519_verify_batch with item i's key taken from a key set: keys[key_idx[i]] -> (n,) uint8, 1 = accept; an index outside
    the key set rejects its item.  numpy inputs (key_idx: uint32) take the host form, CUDA tensors (key_idx: int32, read as
    unsigned) the device form on torch's current stream.  msgs / msg_off / msg_len: as in ed25519_verify_batch."""
    return _run_items("ed25519_verify_keyed", [(sigs, 64, "sigs")], msgs, (), keyed=(keyset, key_idx), msg_off=msg_off, msg_len=msg_len)


def ed25519_verify_keyed_rlc(sigs, keyset, key_idx, msgs, msg_off=None, msg_len=None, return_stats=False):
    """OPT-IN batch verification over a key set (include/eddsa_amd.h): ed25519_verify_batch_rlc with item i's key taken as
    keys[key_idx[i]], for key sets of up to 8192 keys (wider ones run as ed25519_verify_keyed).  Inputs as ed25519_verify_keyed;
    return_stats as ed25519_verify_batch_rlc."""
    return _run_items("ed25519_verify_keyed_rlc", [(sigs, 64, "sigs")], msgs, (), keyed=(keyset, key_idx), msg_off=msg_off, msg_len=msg_len,
                      stats=bool(return_stats))


def ed25519_verify_records(records, sig_off, pub_off, msg_off, msg_len):
    """loop of ed25519_verify over fixed-size records: `records` is an (n, stride) uint8 array (numpy:
    host path, one upload; CUDA tensor: device path) holding each item's 64-byte signature at
    sig_off, 32-byte key at pub_off and msg_len-byte message at msg_off -> (n,) uint8, 1 = accept."""
    lib = library()
    if _is_torch(records):
        import torch
        if records.dtype != torch.uint8 or records.dim() != 2 or not records.is_cuda or not records.is_contiguous():
            raise ValueError("records: expected a contiguous (n, stride) uint8 CUDA tensor")
        n, stride = records.shape
        ok = torch.empty((n,), dtype=torch.uint8, device=records.device)
        _check(lib.ed25519_verify_records_dev(_c_ptr(ok.data_ptr()), _c_ptr(records.data_ptr()), _c_size(stride),
                                              _c_size(sig_off), _c_size(pub_off), _c_size(msg_off), _c_size(msg_len),
                                              _c_size(n), _stream()), "ed25519_verify_records")
        return ok
    records = np.ascontiguousarray(np.asarray(records, dtype=np.uint8))
    if records.ndim != 2:
        raise ValueError("records: expected an (n, stride) uint8 array")
    n, stride = records.shape
    ok = np.zeros((n,), dtype=np.uint8)
    _check(lib.ed25519_verify_records(_np_ptr(ok), _np_ptr(records), _c_size(stride), _c_size(sig_off), _c_size(pub_off),
                                      _c_size(msg_off), _c_size(msg_len), _c_size(n)), "ed25519_verify_records")
    return ok


def ed25519_verify_scattered(data, sig_off, pub_off, msg_off, msg_len):
    """loop of ed25519_verify over items given by byte offsets into one buffer (include/eddsa_amd.h: ed25519_verify_scattered):
    item i's 64-byte signature lies at data[sig_off[i]:], its 32-byte key at data[pub_off[i]:] and its message at
    data[msg_off[i]:msg_off[i] + msg_len[i]]; spans may have any alignment, overlap and be shared between items -> (n,) uint8,
    1 = accept.  numpy (data uint8, the four arrays uint32): the host form, which refuses an item that leaves the buffer; CUDA tensors
    on one device (the four arrays int32, read as unsigned like key_idx, or uint32): the device form on the current stream, where
    such an item gets 0."""
    name = "ed25519_verify_scattered"
    lib = library()
    given = ((sig_off, "sig_off"), (pub_off, "pub_off"), (msg_off, "msg_off"), (msg_len, "msg_len"))
    if _is_torch(data):
        import torch
        data = _torch_check(data, 0, "data")
        for a, nm in given:
            if not _is_torch(a) or a.dtype not in (torch.int32, torch.uint32) or not a.is_cuda or not a.is_contiguous():
                raise ValueError(f"{name}: {nm}: expected contiguous int32 or uint32 offsets on the device")
            if a.device != data.device:
                raise ValueError(f"{name}: {nm} is on {a.device}, data on {data.device}")
            if a.numel() != sig_off.numel():
                raise ValueError(f"{name}: {nm} holds {a.numel()} entries, expected {sig_off.numel()}")
        n = sig_off.numel()
        ok = torch.empty((n,), dtype=torch.uint8, device=data.device)
        _check(lib.ed25519_verify_scattered_dev(_c_ptr(ok.data_ptr()), _c_ptr(data.data_ptr()), _c_size(data.numel()),
                                                *(_c_ptr(a.data_ptr()) for a, _ in given), _c_size(n), _stream()), name)
        return ok
    data = _as_np(data, 0, "data")
    arrs = []
    for a, nm in given:
        a = np.ascontiguousarray(np.asarray(a))
        if a.dtype != np.uint32:
            raise ValueError(f"{name}: {nm}: expected uint32 offsets")
        if arrs and a.size != arrs[0].size:
            raise ValueError(f"{name}: {nm} holds {a.size} entries, expected {arrs[0].size}")
        arrs.append(a)
    n = arrs[0].size
    ok = np.zeros((n,), dtype=np.uint8)
    _check(lib.ed25519_verify_scattered(_np_ptr(ok), _np_ptr(data), _c_size(data.size), *(_np_ptr(a) for a in arrs), _c_size(n)), name)
    return ok


def ed25519_sign_batch(secs, pubs, msgs, msg_off=None, msg_len=None):
    """loop of ed25519_sign (reference lib/eddsa.h:47) -> (n, 64) uint8"""
    return _run_items("ed25519_sign_batch", [(secs, 32, "secs"), (pubs, 32, "pubs")], msgs, (64,), msg_off=msg_off, msg_len=msg_len)


# ---------------------------------------------------------------------------------------------
# Ed25519ctx and Ed25519ph (RFC 8032 5.1; include/eddsa_amd.h): a context of 0..255 bytes, always host bytes
# ---------------------------------------------------------------------------------------------

CONTEXT_MAX = 255
PREHASH_BYTES = 64


def _context(context):
    """-> the context as bytes; ValueError for more than CONTEXT_MAX bytes (before the library is called)"""
    if context is None:
        context = b""
    context = bytes(context)
    if len(context) > CONTEXT_MAX:
        raise ValueError(f"context: {len(context)} bytes, RFC 8032 allows at most {CONTEXT_MAX}")
    return context


def ed25519ctx_sign_batch(secs, pubs, msgs, context, msg_off=None, msg_len=None):
    """Ed25519ctx signatures (RFC 8032 5.1, dom2 flag 0) of the messages under `context` (bytes, 0..255) -> (n, 64) uint8;
    messages as in ed25519_sign_batch"""
    return _run_items("ed25519ctx_sign_batch", [(secs, 32, "secs"), (pubs, 32, "pubs")], msgs, (64,), msg_off=msg_off, msg_len=msg_len,
                      context=_context(context))


def ed25519ctx_verify_batch(sigs, pubs, msgs, context, msg_off=None, msg_len=None):
    """Ed25519ctx verdicts -> (n,) uint8, 1 = accept; the off-curve mode and the verify policy apply as in ed25519_verify_batch"""
    return _run_items("ed25519ctx_verify_batch", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], msgs, (), msg_off=msg_off, msg_len=msg_len,
                      context=_context(context))


def ed25519ph_sign_batch(secs, pubs, prehashes, context=b""):
    """Ed25519ph signatures (dom2 flag 1) over caller-supplied prehashes[i] = SHA-512(M_i), 64 bytes per item as
    hashlib.sha512(M).digest() returns them: the library never sees M -> (n, 64) uint8"""
    return _run_items("ed25519ph_sign_batch", [(secs, 32, "secs"), (pubs, 32, "pubs")], prehashes, (64,), fixed=PREHASH_BYTES,
                      data_name="prehashes", context=_context(context))


def ed25519ph_verify_batch(sigs, pubs, prehashes, context=b""):
    """Ed25519ph verdicts over caller-supplied prehashes (see ed25519ph_sign_batch) -> (n,) uint8, 1 = accept"""
    return _run_items("ed25519ph_verify_batch", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], prehashes, (), fixed=PREHASH_BYTES,
                      data_name="prehashes", context=_context(context))


# ---------------------------------------------------------------------------------------------
# key sets: the digest, Ed25519ctx and Ed25519ph forms (include/eddsa_amd.h)
# ---------------------------------------------------------------------------------------------

def ed25519_verify_keyed_digests(sigs, keyset, key_idx, digests):
    """ed25519_verify_digests with item i's key taken from a key set: the caller vouches that digests[i] =
    SHA-512(R_i || keys[key_idx[i]] || M_i) (64 bytes per item) -> (n,) uint8, 1 = accept; an index outside the key set rejects
    its item.  A comb key set takes the comb route.  Inputs as ed25519_verify_keyed (numpy: host form, CUDA tensors: device form)."""
    return _run_items("ed25519_verify_keyed_digests", [(sigs, 64, "sigs")], digests, (), keyed=(keyset, key_idx), fixed=64, data_name="digests")


def ed25519_verify_keyed_digests_rlc(sigs, keyset, key_idx, digests, return_stats=False):
    """ed25519_verify_keyed_rlc from caller-supplied digests (see ed25519_verify_keyed_digests): the verdicts and statistics of
    ed25519_verify_digests_rlc over keys[key_idx]; key sets of more than 8192 keys run as ed25519_verify_keyed_digests."""
    return _run_items("ed25519_verify_keyed_digests_rlc", [(sigs, 64, "sigs")], digests, (), keyed=(keyset, key_idx), fixed=64,
                      data_name="digests", stats=bool(return_stats))


def ed25519ctx_verify_keyed(sigs, keyset, key_idx, msgs, context, msg_off=None, msg_len=None):
    """ed25519ctx_verify_batch with item i's key taken from a key set -> (n,) uint8, 1 = accept; `context`: host bytes, 0..255;
    messages as in ed25519_verify_keyed"""
    return _run_items("ed25519ctx_verify_keyed", [(sigs, 64, "sigs")], msgs, (), keyed=(keyset, key_idx), msg_off=msg_off, msg_len=msg_len,
                      context=_context(context))


def ed25519ph_verify_keyed(sigs, keyset, key_idx, prehashes, context=b""):
    """ed25519ph_verify_batch with item i's key taken from a key set: prehashes[i] = SHA-512(M_i), 64 bytes per item
    -> (n,) uint8, 1 = accept"""
    return _run_items("ed25519ph_verify_keyed", [(sigs, 64, "sigs")], prehashes, (), keyed=(keyset, key_idx), fixed=PREHASH_BYTES,
                      data_name="prehashes", context=_context(context))


# ---------------------------------------------------------------------------------------------
# signer sets (include/eddsa_amd.h: eddsa_amd_signer): secret keys registered once, signed with by key index
# ---------------------------------------------------------------------------------------------

SIGNER_MAX_KEYS = 1 << 20                      # EDDSA_AMD_SIGNER_MAX_KEYS


class Signer:
    """A signer set (include/eddsa_amd.h: eddsa_amd_signer): secret keys registered once - per key the scalar a mod l, the prefix
    and the public key it derives, in HBM - for ed25519_sign_keyed and its ctx / ph forms.  Immutable; lives until close() (or the
    end of a `with` block), also across shutdown(); close() zeroes the secrets on the device."""

    def __init__(self, handle):
        self._h = handle

    def _handle(self):
        if self._h is None:
            raise ValueError("Signer: already closed")
        return self._h

    @property
    def count(self):
        lib = library()
        lib.eddsa_amd_signer_count.restype = ctypes.c_size_t
        return int(lib.eddsa_amd_signer_count(self._handle()))

    @property
    def device(self):
        return int(library().eddsa_amd_signer_device(self._handle()))

    def pubs(self):
        """the public keys the set derived, (count, 32) uint8: what a verifier registers (keyset_create(signer.pubs()))"""
        out = np.zeros((self.count, 32), dtype=np.uint8)
        _check(library().eddsa_amd_signer_pubs(self._handle(), _np_ptr(out)), "eddsa_amd_signer_pubs")
        return out

    def close(self):
        if self._h is not None:
            library().eddsa_amd_signer_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def signer_create(secs=None, expanded=None):
    """secs: count x 32 bytes of seeds, or expanded: count x 64 bytes of scalar | prefix (the scalar is used mod l, not clamped);
    numpy / bytes, host memory; exactly one of the two -> Signer, on the default device."""
    if (secs is None) == (expanded is None):
        raise ValueError("signer_create: pass either secs or expanded")
    lib = library()
    h = _c_ptr()
    name, keys, width = ("eddsa_amd_signer_create", secs, 32) if expanded is None else ("eddsa_amd_signer_create_expanded", expanded, 64)
    keys = _as_np(keys, width, "secs" if expanded is None else "expanded")
    _check(getattr(lib, name)(ctypes.byref(h), _np_ptr(keys), _c_size(keys.size // width)), name)
    return Signer(h)


def ed25519_sign_keyed(signer, key_idx, msgs, msg_off=None, msg_len=None):
    """ed25519_sign_batch with item i's key taken from a signer set: the signatures of (key key_idx[i], message i) -> (n, 64) uint8.
    numpy inputs take the host form (an index outside the set: EddsaAmdError, nothing is signed), CUDA tensors the device form
    (such an item gets 64 zero bytes).  msgs / msg_off / msg_len: as in ed25519_sign_batch."""
    return _run_items("ed25519_sign_keyed", [], msgs, (64,), keyed=(signer, key_idx), msg_off=msg_off, msg_len=msg_len)


def ed25519ctx_sign_keyed(signer, key_idx, msgs, context, msg_off=None, msg_len=None):
    """ed25519ctx_sign_batch with item i's key taken from a signer set -> (n, 64) uint8; `context`: host bytes, 0..255"""
    return _run_items("ed25519ctx_sign_keyed", [], msgs, (64,), keyed=(signer, key_idx), msg_off=msg_off, msg_len=msg_len,
                      context=_context(context))


def ed25519ph_sign_keyed(signer, key_idx, prehashes, context=b""):
    """ed25519ph_sign_batch with item i's key taken from a signer set: prehashes[i] = SHA-512(M_i), 64 bytes per item -> (n, 64) uint8"""
    return _run_items("ed25519ph_sign_keyed", [], prehashes, (64,), keyed=(signer, key_idx), fixed=PREHASH_BYTES, data_name="prehashes",
                      context=_context(context))


# ---------------------------------------------------------------------------------------------
# several devices in one process (include/eddsa_amd.h: *_multi), after init_devices()
# ---------------------------------------------------------------------------------------------

def ed25519_verify_batch_multi(sigs, pubs, msgs, msg_off=None, msg_len=None):
    """ed25519_verify_batch over the device set: contiguous shards, one host thread per device"""
    return _run_items("ed25519_verify_batch_multi", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], msgs, (), msg_off=msg_off, msg_len=msg_len,
                      dev=False, sizes_first=True)


def ed25519_verify_digests_multi(sigs, pubs, digests):
    """ed25519_verify_digests over the device set (host arrays): contiguous shards, one host thread per device"""
    return _run_items("ed25519_verify_digests_multi", [(sigs, 64, "sigs"), (pubs, 32, "pubs")], digests, (), fixed=64, data_name="digests",
                      dev=False)


def ed25519_sign_batch_multi(secs, pubs, msgs, msg_off=None, msg_len=None):
    return _run_items("ed25519_sign_batch_multi", [(secs, 32, "secs"), (pubs, 32, "pubs")], msgs, (64,), msg_off=msg_off, msg_len=msg_len,
                      dev=False, sizes_first=True)


def x25519_batch_multi(scalars, points):
    scalars = _as_np(scalars, 32, "scalars"); points = _as_np(points, 32, "points")
    n = scalars.size // 32
    if points.size // 32 != n:
        raise ValueError("x25519_batch_multi: scalars and points disagree on the batch size")
    out = np.zeros((n, 32), dtype=np.uint8)
    _check(library().x25519_batch_multi(_np_ptr(out), _np_ptr(scalars), _np_ptr(points), _c_size(n)), "x25519_batch_multi")
    return out


def ed25519_verify_batch_multi_dev(sigs, pubs, msgs, msg_len, n_total):
    """sigs[d], pubs[d], msgs[d]: CUDA tensors holding shard d (shard_bounds(n_total, d, G)) on device d
    of the set.  Returns one (n_total,) uint8 tensor per device, each holding the WHOLE verdict vector
    after the RCCL all-gather; work is enqueued on each device's current torch stream."""
    import torch
    g = device_count()
    if not (len(sigs) == len(pubs) == len(msgs) == g):
        raise ValueError(f"expected one shard per device of the set ({g})")
    outs, streams = [], []
    from .sharding import shard_bounds
    for d in range(g):
        _torch_check(sigs[d], 64, "sigs"); _torch_check(pubs[d], 32, "pubs"); _torch_check(msgs[d], 0, "msgs")
        # the C entry point trusts its pointers: a short shard would be read out of bounds on the device, a shard on
        # another device than the set's d-th would be launched on the wrong stream
        lo, hi = shard_bounds(n_total, d, g)
        if sigs[d].numel() != 64 * (hi - lo) or pubs[d].numel() != 32 * (hi - lo) or msgs[d].numel() != int(msg_len) * (hi - lo):
            raise ValueError(f"shard {d}: expected {hi - lo} items (shard_bounds({n_total}, {d}, {g})) in sigs, pubs and msgs")
        want_dev = int(library().eddsa_amd_device_at(d))
        for t, nm in ((sigs[d], "sigs"), (pubs[d], "pubs"), (msgs[d], "msgs")):
            if t.device.index != want_dev:
                raise ValueError(f"shard {d}: {nm} lives on cuda:{t.device.index}, the set's device {d} is cuda:{want_dev}")
        outs.append(torch.empty((n_total,), dtype=torch.uint8, device=sigs[d].device))
        streams.append(torch.cuda.current_stream(sigs[d].device).cuda_stream)
    P = ctypes.c_void_p * g
    _check(library().ed25519_verify_batch_multi_dev(P(*[o.data_ptr() for o in outs]), P(*[t.data_ptr() for t in sigs]),
                                                    P(*[t.data_ptr() for t in pubs]), P(*[t.data_ptr() for t in msgs]),
                                                    _c_size(msg_len), _c_size(n_total), P(*streams)),
           "ed25519_verify_batch_multi_dev")
    return outs


# ---------------------------------------------------------------------------------------------
# the eddsa.h surface (single items; bytes in, bytes out), reference lib/eddsa.h:44-113
# ---------------------------------------------------------------------------------------------

def _b(x, n, name):
    x = bytes(x)
    if len(x) != n:
        raise ValueError(f"{name}: expected {n} bytes, got {len(x)}")
    return x


def _single(name, out_bytes, *fixed, data=False):
    """the eddsa.h function `name`: fixed = (argument, bytes) of each fixed-width input; data: a message of any length
    follows them; out_bytes bytes come back (0: the C function's bool)"""
    names = [nm for nm, _ in fixed] + ["data"] * data

    def fn(*args, **kw):
        given = dict(zip(names, args), **kw)
        if len(args) > len(names) or len(given) != len(args) + len(kw) or set(given) != set(names):
            raise TypeError(f"{name}({', '.join(names)}): got {len(args)} positional arguments and keywords {sorted(kw)}")
        tail = [bytes(given["data"])] if data else []
        f = getattr(library(), name)
        cargs = [_b(given[nm], w, nm) for nm, w in fixed] + tail + [_c_size(len(d)) for d in tail]
        if not out_bytes:
            return bool(f(*cargs))
        out = ctypes.create_string_buffer(out_bytes)
        f(out, *cargs)
        return out.raw
    fn.__name__ = fn.__qualname__ = name
    return fn


ed25519_genpub = _single("ed25519_genpub", 32, ("sec", 32))
ed25519_sign = _single("ed25519_sign", 64, ("sec", 32), ("pub", 32), data=True)
ed25519_verify = _single("ed25519_verify", 0, ("sig", 64), ("pub", 32), data=True)
x25519_base = _single("x25519_base", 32, ("scalar", 32))
x25519 = _single("x25519", 32, ("scalar", 32), ("point", 32))
pk_ed25519_to_x25519 = _single("pk_ed25519_to_x25519", 32, ("pub", 32))
sk_ed25519_to_x25519 = _single("sk_ed25519_to_x25519", 32, ("sec", 32))
# obsolete names kept by the reference (lib/eddsa.h:92-113)
eddsa_genpub = _single("eddsa_genpub", 32, ("sec", 32))
eddsa_sign = _single("eddsa_sign", 64, ("sec", 32), ("pub", 32), data=True)
eddsa_verify = _single("eddsa_verify", 0, ("sig", 64), ("pub", 32), data=True)
DH = _single("DH", 32, ("sec", 32), ("point", 32))
eddsa_pk_eddsa_to_dh = _single("eddsa_pk_eddsa_to_dh", 32, ("pub", 32))
eddsa_sk_eddsa_to_dh = _single("eddsa_sk_eddsa_to_dh", 32, ("sec", 32))
