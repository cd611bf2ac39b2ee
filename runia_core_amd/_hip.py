"""ctypes binding of ``librunia_hip.so`` (C ABI in ``include/runia_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every
numerical stage of the scoring path is a kernel of the shared library.  There is
NO CPU fallback: without the library or without a GPU the wrappers raise.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch  # imported before the library so that both share one HIP runtime

from . import config as _config

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "librunia_hip.so")
_lib: Optional[ctypes.CDLL] = None

_HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "runia_hip.h")


class RuniaHipError(RuntimeError):
    pass


# value types of the C ABI; every parameter declared with `*` or `[]` is an address (c_void_p)
_C_TYPES = {"void": None, "int": c_int, "int64_t": c_int64, "size_t": c_size_t, "uint64_t": c_uint64, "uint32_t": c_uint32,
            "unsigned": c_uint32, "double": c_double, "float": c_float, "runia_stream_t": c_void_p}
# host out-parameters: the only entries whose ctypes type says more than the header (name -> {parameter index: type})
_HOST_OUT_PARAMS = {
    "runia_p2p_alloc": {2: ctypes.POINTER(c_void_p)},
    "runia_p2p_open": {1: ctypes.POINTER(c_void_p)},
    "runia_p2p_all_gather": {3: ctypes.POINTER(c_void_p)},
    "runia_p2p_status": {1: ctypes.POINTER(c_int)},
}


def _c_type(decl: str, symbol: str, result: bool = False):
    """ctypes type of one parameter declaration (``const float* x``, ``int64_t N``, ``double w[4]``) or of a return type."""
    words = [w for w in re.sub(r"[*\[\]]", " ", decl).split() if w != "const"]
    if "*" in decl or "[" in decl:
        if not result:
            return c_void_p
        if words == ["char"]:
            return c_char_p
    elif words and words[0] in _C_TYPES and len(words) <= (1 if result else 2):
        return _C_TYPES[words[0]]
    raise RuniaHipError(f"include/runia_hip.h: {symbol}: no ctypes type for {decl.strip()!r}")


def _macro_int(body: str) -> int:
    """Value of an integer macro body: ``n``, ``(-n)`` or ``(a << b)``; anything else raises ValueError."""
    m = re.fullmatch(r"\(?\s*(-?\d+)\s*(?:<<\s*(\d+)\s*)?\)?", body.strip())
    if not m or body.count("(") != body.count(")"):
        raise ValueError(f"not an integer macro body: {body!r}")
    return int(m.group(1)) << int(m.group(2) or 0)


def _parse_header(text: str):
    """``(signatures, macros)`` of a C header text: ``name -> (restype, [argtypes])`` for every ``ret runia_*(args);`` and
    ``name -> int`` for every ``#define RUNIA_*`` whose body is an integer.  A type outside ``_C_TYPES`` raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    macros = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RUNIA_\w+)(.*)$", text, flags=re.M):
        try:
            macros[name] = _macro_int(body)
        except ValueError:  # include guard, function-like macros
            pass
    signatures = {}
    for ret, name, params in re.findall(r"([\w \t\n*]+?)\b(runia_\w+)\s*\(([^()]*)\)\s*;", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_c_type(ret, name, result=True), [_c_type(p, name) for p in params])
    for name, fixed in _HOST_OUT_PARAMS.items():
        for i, t in fixed.items():
            if name in signatures:
                signatures[name][1][i] = t
    return signatures, macros


def _read_header():
    try:
        with open(_HEADER_PATH) as f:
            return _parse_header(f.read())
    except OSError as e:
        raise RuniaHipError(f"cannot read the C ABI header {os.path.normpath(_HEADER_PATH)}: {e}") from e


# name -> (restype, argtypes) of every entry point, and the integer RUNIA_* macros: both read from include/runia_hip.h
_SIGNATURES, _HEADER_MACROS = _read_header()


class CounterDraws(NamedTuple):
    """DropBlock draws made inside the keep-flag kernel by the counter generator (Philox4x32-10, csrc/philox.hpp):
    image i of the batch uses image id ``first_image + i`` of the stream keyed by ``seed``.  ``redraw_dead_layers``:
    a drop layer that removes the whole map (NaN upstream as well) draws again from the image's next counter block."""

    seed: int
    first_image: int = 0
    redraw_dead_layers: bool = False


def library_path() -> str:
    return _LIB_PATH


def load_library() -> ctypes.CDLL:
    """Load the shared library and declare every C-ABI signature.  Works without a GPU."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            # a missing build artefact is built, never replaced: there is no other implementation to fall back to
            import subprocess

            try:
                subprocess.run(["make", "-C", os.path.join(os.path.dirname(_LIB_PATH), "csrc"), "-j8", "-s"], check=True,
                               stdout=subprocess.DEVNULL)
            except Exception:
                pass
        if not os.path.exists(_LIB_PATH):
            raise RuniaHipError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  runia_core_amd has no CPU fallback."
            )
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def require_gpu() -> torch.device:
    """The scoring path is HIP-only.  Fail loudly when it cannot run."""
    lib = load_library()
    if not torch.cuda.is_available() or lib.runia_device_count() < 1:
        raise RuniaHipError(
            "runia_core_amd: no HIP device visible (torch.cuda.is_available() is False). "
            "The scoring hot path runs only as HIP kernels on MI355X; there is no CPU fallback."
        )
    return torch.device("cuda", torch.cuda.current_device())


def array_fingerprint(a):
    """Cheap identity of a fitted array (address, shape, dtype): reassigning or refitting gives a new array, so caches of
    device copies keyed on it are rebuilt instead of going stale.  (In-place edits of the same buffer are not seen.)"""
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return ("t", a.data_ptr(), tuple(a.shape), str(a.dtype))
    a = np.asarray(a)
    return ("n", a.__array_interface__["data"][0], a.shape, a.dtype.str)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().runia_error_string(rc).decode()
        raise RuniaHipError(f"{what} failed: {msg} (code {rc})")


def _cuda_tensors(value):
    """CUDA tensors inside an argument (the argument itself, or the members of a tuple / list such as a packed state)."""
    if getattr(value, "is_cuda", False) is True:
        yield value
    elif isinstance(value, (tuple, list)):
        for v in value:
            yield from _cuda_tensors(v)


def resolve_device(args, kwargs, exempt=()):
    """The one device a wrapper call runs on: that of its CUDA tensor arguments (``exempt``: names the wrapper moves to
    the first tensor's device itself).  Tensors on different devices raise ``RuniaHipError`` - a kernel launched with
    pointers of two GPUs would fault or, worse, read peer memory silently.  No CUDA tensor -> None (the current device).
    (On the path of every wrapper call - 1 500 per harness sweep: plain loops, no intermediate lists.)"""
    dev, first = None, None
    i = -1
    for value in args:
        i += 1
        if value is None or i in exempt:
            continue
        if type(value) is torch.Tensor:
            if not value.is_cuda:
                continue
            d = value.device
            if dev is None:
                dev, first = d, i
            elif d != dev:
                _raise_two_devices(dev, first, d, i)
        elif isinstance(value, (tuple, list)) or getattr(value, "is_cuda", False) is True:  # packed states, tensor subclasses
            for t in _cuda_tensors(value):
                if dev is None:
                    dev, first = t.device, i
                elif t.device != dev:
                    _raise_two_devices(dev, first, t.device, i)
    for name, value in kwargs.items():
        if value is None or name in exempt:
            continue
        for t in _cuda_tensors(value):
            if dev is None:
                dev, first = t.device, name
            elif t.device != dev:
                _raise_two_devices(dev, first, t.device, name)
    return dev


def _raise_two_devices(dev, first, other, name):
    raise RuniaHipError(f"tensor arguments sit on different devices ({dev} for argument {first!r}, {other} for "
                        f"argument {name!r}): move them to one GPU before the call")


def _device_guard(*exempt):
    """Run the wrapper with the arguments' GPU as the current device: the launch stream (``_stream``), the workspaces
    and ``require_gpu()`` then all belong to the device the operands live on, whatever ``torch.cuda.current_device()``
    was (the reference's users do ``model.to("cuda:1")``, inference/abstract_classes.py:250-255)."""
    import functools
    import inspect

    def wrap(fn):
        names = list(inspect.signature(fn).parameters)
        skip = {names.index(e) for e in exempt if e in names} | set(exempt)

        @functools.wraps(fn)
        def guarded(*args, **kwargs):
            dev = resolve_device(args, kwargs, skip)
            if dev is None or dev.index is None or dev.index == torch.cuda.current_device():
                return fn(*args, **kwargs)
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)

        return guarded

    return wrap


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The current device's current stream as the C ABI's ``runia_stream_t`` (torch's raw-stream query where this build has it:
    no ``torch.cuda.Stream`` object per wrapper call - 2 400 of them per harness sweep)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# element dtype of a tensor read in place -> the `dtype` code of the C ABI (csrc/elem.hpp)
ELEM_DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def launch(name: str, *args) -> None:
    """Call the entry point ``name`` with ``args`` and the current stream (always its last parameter); a non-zero code raises
    ``RuniaHipError`` naming that symbol.  It never asks for the GPU: ``require_gpu()`` stays where each wrapper has it, because
    which refusal comes first on a box without a device is part of every wrapper's contract."""
    rc = getattr(load_library(), name)(*args, _raw_stream(torch.cuda.current_device()) if _raw_stream is not None else _stream())
    if rc != 0:
        _check(rc, name)


def call(name: str, *args) -> None:
    """``launch`` for the entry points without a stream parameter (the p2p family, ``runia_time_next_launch``,
    ``runia_pacmap_phase_weights``)."""
    rc = getattr(load_library(), name)(*args)
    if rc != 0:
        _check(rc, name)


def query(name: str, *args) -> int:
    """The value of an entry point that returns a number, not an error code (``*_workspace_bytes``, ``*_bytes``,
    ``*_supported``, ``runia_eigh_block_padded``, ``runia_knn_piece_products``), as a Python int."""
    return int(getattr(load_library(), name)(*args))


def workspace(nbytes: int, device, floor: int = 16) -> torch.Tensor:
    """Uninitialised scratch of ``max(nbytes, floor)`` bytes for one call (stream-ordered: the caching allocator hands the block
    to the next call on the stream).  Blocks are 512-byte aligned whatever the kernel reads them as."""
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)


def _draws(rand: Optional[torch.Tensor], n: int, n_mc: int, h: int, w: int, copy: bool = True):
    """Check explicit DropBlock draws ([n_mc, H, W] shared by the images, or [N, n_mc, H, W]) -> ``(rand, image stride in
    elements)``; ``(None, 0)`` without draws.  ``copy=False`` refuses draws that are not contiguous instead of copying them."""
    if rand is None:
        return None, 0
    assert rand.is_cuda and rand.dtype == torch.float32 and (copy or rand.is_contiguous())
    if copy:
        rand = rand.contiguous()
    if rand.dim() == 4:
        assert rand.shape == (n, n_mc, h, w)
        return rand, n_mc * h * w
    assert rand.shape == (n_mc, h, w)
    return rand, 0


def _image_slices(n: int):
    """``(done, m)``: slices of at most 65 535 images, the grid limit of the sampler kernels."""
    for done in range(0, n, 65535):
        yield done, min(65535, n - done)


class _UploadCache(threading.local):
    depth = 0
    entries = None


_upload_cache = _UploadCache()
_UPLOAD_CACHE_MIN_BYTES = 1 << 20


@contextlib.contextmanager
def upload_cache():
    """While the context is open (re-entrant, per thread), ``to_device`` of a C-contiguous host ndarray of at least 1 MB is done once
    per (buffer address, shape, dtype, target dtype): later calls return the same device tensor.  For loops that hand the SAME
    host arrays to many setup / postprocess calls (``evaluation.baselines.calculate_all_baselines(device_resident=True)``: the
    training features would otherwise be uploaded by eight fits, each split by every baseline).  The arrays must not be written to
    while the context is open (the postprocessors never do: inputs are read-only by contract); the cache holds a reference to
    every array it has seen and drops everything when the outermost context closes.  The tensors are shared: read-only as well."""
    c = _upload_cache
    if c.depth == 0:
        c.entries = {}
    c.depth += 1
    try:
        yield
    finally:
        c.depth -= 1
        if c.depth == 0:
            c.entries = None


def to_device(a, dtype: torch.dtype) -> torch.Tensor:
    """Host ndarray / tensor -> contiguous device tensor of ``dtype`` (H2D copy if needed; see ``upload_cache``)."""
    dev = require_gpu()
    if isinstance(a, np.ndarray):
        c = _upload_cache
        if c.depth > 0 and a.flags.c_contiguous and a.nbytes >= _UPLOAD_CACHE_MIN_BYTES:
            key = (a.__array_interface__["data"][0], a.shape, a.dtype.str, dtype, str(dev))
            hit = c.entries.get(key)
            if hit is None:
                hit = (a, torch.from_numpy(a).to(device=dev, dtype=dtype, non_blocking=False).contiguous())
                c.entries[key] = hit
            return hit[1]
        t = torch.from_numpy(np.ascontiguousarray(a))
    elif isinstance(a, torch.Tensor):
        t = a.detach()
    else:
        t = torch.as_tensor(np.asarray(a))
    return t.to(device=dev, dtype=dtype, non_blocking=False).contiguous()


_PINNED_MIN, _PINNED_MAX = 1 << 16, 1 << 30


def to_host(t: torch.Tensor) -> np.ndarray:
    """Device tensor -> host ndarray (the ``.cpu().numpy()`` of every API that returns arrays, as the reference's do).
    Results between 64 KB and 1 GB land in page-locked memory from torch's caching host allocator and the ndarray is a
    view of it: a D2H copy into freshly allocated pageable memory runs at ~2 GB/s on this platform (first-touch page
    faults; the 41 MB of entropies of a 10 000-image batch took 19 ms, 200 x the kernels that made them), into a
    recycled pinned block at the link rate.  The block returns to the allocator's cache when the array is released."""
    if not t.is_cuda:
        return t.detach().numpy()
    t = t.detach().contiguous()
    nbytes = t.numel() * t.element_size()
    if nbytes < _PINNED_MIN or nbytes > _PINNED_MAX:
        return t.cpu().numpy()
    try:
        out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    except RuntimeError:  # locked-memory limit reached, fragmentation: the pageable copy is slower, never wrong
        return t.cpu().numpy()
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return out.numpy()


# --------------------------------------------------------------------------------------
# stage wrappers: device tensors in, device tensors out, stream-ordered, no sync
# --------------------------------------------------------------------------------------
@_device_guard()
def mc_stack(x: torch.Tensor, rand: Optional[torch.Tensor], n_mc: int, drop_prob: float, block_size: int) -> torch.Tensor:
    """x [N,C,H,W] f32, rand [n_mc,H,W] (shared) or [N,n_mc,H,W] f32 -> [N*n_mc, C] f32."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n, c, h, w = x.shape
    if isinstance(rand, CounterDraws):
        rand = _explicit_counter_draws(rand, n, n_mc, h, w)
    rand, stride = _draws(rand, n, n_mc, h, w)
    out = torch.empty((n * n_mc, c), dtype=torch.float32, device=x.device)
    table_path = n_mc >= 2 and bool(query("runia_mc_entropy_supported", h, w, n_mc, 5)) and (x.data_ptr() % 16 == 0 or (h * w) % 4)
    if table_path:
        ws_bytes = query("runia_mc_entropy_workspace_bytes", min(65535, n), h, w, n_mc)
        ws = workspace(ws_bytes, x.device)
    for done, m in _image_slices(n):
        xp, op = x.data_ptr() + done * c * h * w * 4, out.data_ptr() + done * n_mc * c * 4
        rp = None if rand is None else rand.data_ptr() + done * stride * 4
        if table_path:
            launch("runia_mc_stack_table_f32", xp, rp, stride, op, ws.data_ptr(), ws_bytes, m, c, h, w, n_mc, float(drop_prob),
                   int(block_size))
        else:
            launch("runia_mc_stack_f32", xp, rp, stride, op, m, c, h, w, n_mc, float(drop_prob), int(block_size))
    return out


def _explicit_counter_draws(ticket: CounterDraws, n: int, n_mc: int, h: int, w: int) -> torch.Tensor:
    """Counter draws written out for the kernels that read draws from memory.  The redraw of fully dropped maps lives in
    the keep-flag kernel (fused table path: 2x2 / 4x4 / 7x7 / 8x8 maps): it cannot be honoured here, so it is refused
    rather than silently ignored."""
    if ticket.redraw_dead_layers:
        raise RuniaHipError("CounterDraws(redraw_dead_layers=True) is implemented by the keep-flag kernel of the fused "
                            "sampler + entropy path (maps of 2x2, 4x4, 7x7, 8x8); this call takes the explicit-draw kernels")
    return mc_draws(n, n_mc, h, w, ticket.seed, ticket.first_image)


def mc_draws(n: int, n_mc: int, h: int, w: int, seed: int, first_image: int = 0) -> torch.Tensor:
    """The counter generator's draws written out: [n, n_mc, h, w] f32 in [0, 1) (same values the counter entry points
    use inside the keep-flag kernel)."""
    dev = require_gpu()
    out = torch.empty((n, n_mc, h, w), dtype=torch.float32, device=dev)
    launch("runia_mc_draws_f32", out.data_ptr(), n, n_mc, h, w, int(seed) & (2**64 - 1), int(first_image))
    return out


@_device_guard()
def mc_drop_flat(x: torch.Tensor, rand: Optional[torch.Tensor], n_mc: int, drop_prob: float, block_size: int) -> torch.Tensor:
    """``layer_type="FC"/"RPN"`` form of the sampler: x [N,C,H,W] f32 -> [N*n_mc, C*H*W] f32 (no fullmean)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n, c, h, w = x.shape
    if isinstance(rand, CounterDraws):
        rand = _explicit_counter_draws(rand, n, n_mc, h, w)
    rand, stride = _draws(rand, n, n_mc, h, w)
    e = c * h * w
    out = torch.empty((n * n_mc, e), dtype=torch.float32, device=x.device)
    for done, m in _image_slices(n):
        rp = None if rand is None else rand.data_ptr() + done * stride * 4
        launch("runia_mc_drop_flat_f32", x.data_ptr() + done * e * 4, rp, stride, out.data_ptr() + done * n_mc * e * 4, m, c, h,
               w, n_mc, float(drop_prob), int(block_size))
    return out


@_device_guard()
def map_reduce(x: torch.Tensor, h: int, w: int, mode: str) -> torch.Tensor:
    """x [..., h*w] f32 seen as maps of h x w -> ``mode="mean"``: mean over w, [maps, h]; ``mode="std"``: std over the
    rows of the per-row stds, [maps] (the reductions of ``get_mean_or_fullmean_ls_sample(., "mean")`` and
    ``get_std_ls_sample`` upstream)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.numel() % (h * w) == 0 and mode in ("mean", "std")
    x = x.contiguous()
    maps = x.numel() // (h * w)
    out = torch.empty((maps, h) if mode == "mean" else (maps,), dtype=torch.float32, device=x.device)
    launch("runia_map_reduce_f32", x.data_ptr(), out.data_ptr(), maps, h, w, 0 if mode == "mean" else 1)
    return out


_MCD_MODES = {m: _HEADER_MACROS["RUNIA_MCD_" + m.upper()] for m in ("fullmean", "mean", "avgpool", "copy")}


def mcd_row_width(shape, mode: str, avg_pooling_parameters=None) -> int:
    """Width D of the row ``mcd_reduce_rows`` writes per image for an activation of ``shape`` (2-D or 4-D)."""
    assert mode in _MCD_MODES, f"mode must be one of {sorted(_MCD_MODES)}"
    assert len(shape) in (2, 4), "the activation must be (B, F) or (B, C, H, W)"
    c, h, w = (int(shape[1]), 1, 1) if len(shape) == 2 else (int(shape[1]), int(shape[2]), int(shape[3]))
    if mode == "fullmean":
        return c
    if mode == "mean":
        return c * h
    if mode == "copy":
        return c * h * w
    assert avg_pooling_parameters is not None and len(avg_pooling_parameters) == 3, \
        "Three parameters are needed for average pooling"
    k, st, p = (int(v) for v in avg_pooling_parameters)
    assert k > 0 and st > 0 and 0 <= 2 * p <= k, "pad should be at most half of the kernel size"
    assert h + 2 * p >= k and w + 2 * p >= k, "the pooling window is larger than the padded map"
    return c * ((h + 2 * p - k) // st + 1) * ((w + 2 * p - k) // st + 1)


@_device_guard()
def mcd_reduce_rows(x: torch.Tensor, table: torch.Tensor, mode: str, row0: int = 0, row_step: int = 1,
                    avg_pooling_parameters=None) -> torch.Tensor:
    """Reduce the hooked activation ``x`` ((B, C, H, W) or (B, F); f32 / f16 / bf16; any strides, read in place) and write
    the row of image ``b`` into ``table[row0 + b * row_step, :D]`` (``table`` f32, row-major, ``table.shape[1] >= D``).
    ``mode``: ``"fullmean"`` (D = C), ``"mean"`` (over W, D = C*H), ``"avgpool"`` with ``avg_pooling_parameters =
    (kernel, stride, padding)`` (``avg_pool2d`` defaults, D = C*Ho*Wo), ``"copy"`` (the flattened activation).  One
    launch on the current stream; the other rows and the columns from D on keep their contents.  Returns ``table``."""
    # shapes and dtypes first, then the devices: every refusal comes before the library is touched
    assert isinstance(x, torch.Tensor) and isinstance(table, torch.Tensor)
    assert x.dtype in ELEM_DTYPE_CODES, f"unsupported activation dtype {x.dtype} (float32, float16, bfloat16)"
    assert table.dtype == torch.float32 and table.dim() == 2 and (table.shape[0] <= 1 or table.stride(0) >= table.shape[1]) \
        and (table.shape[1] <= 1 or table.stride(1) == 1), "the table must be a row-major float32 matrix"
    d = mcd_row_width(x.shape, mode, avg_pooling_parameters)
    assert table.shape[1] >= d, f"the table is too narrow: {table.shape[1]} columns for rows of {d} values"
    b = int(x.shape[0])
    row0, row_step = int(row0), int(row_step)
    assert row0 >= 0 and row_step >= 1 and (b == 0 or row0 + (b - 1) * row_step < table.shape[0]), \
        f"rows {row0} + b * {row_step}, b < {b}, leave the table of {table.shape[0]} rows"
    assert x.is_cuda, "the activation must be a device tensor"
    assert table.is_cuda and table.device == x.device, "the table must be on the activation's device"
    require_gpu()
    if b == 0:
        return table
    if x.dim() == 2:
        x = x[:, :, None, None]
    k, st, p = (int(v) for v in avg_pooling_parameters) if mode == "avgpool" else (0, 0, 0)
    ld = int(table.stride(0)) if table.shape[0] > 1 else max(int(table.stride(0)), int(table.shape[1]))
    launch("runia_mcd_reduce_rows", x.data_ptr(), ELEM_DTYPE_CODES[x.dtype], b, x.shape[1], x.shape[2], x.shape[3], x.stride(0),
           x.stride(1), x.stride(2), x.stride(3), _MCD_MODES[mode], k, st, p, table.data_ptr(), table.shape[0], ld, row0,
           row_step)
    return table


_RAGGED_MODES = {m: _HEADER_MACROS["RUNIA_RAGGED_" + m.upper()] for m in ("copy", "log_eps")}


@_device_guard()
def ragged_rows(tensors, mode: str = "copy", out: Optional[torch.Tensor] = None, return_segments: bool = False):
    """``torch.cat(tensors, dim=0)`` of 2-D device tensors of one width and dtype (f32 / f16 / bf16; any strides, read in place;
    tensors of 0 rows allowed) in ONE launch: the descriptors and the prefix sum of the row counts go up as one copy.
    ``mode="log_eps"`` writes ``torch.log(t + 1e-10)`` of every tensor instead.  ``out``: an existing row-major table of that
    dtype with ``sum(rows)`` rows and at least D columns (the columns from D on keep their contents).  Returns the table, and
    with ``return_segments`` also the int32 index of the tensor every row came from.  No host synchronisation."""
    assert mode in _RAGGED_MODES, f"mode must be one of {sorted(_RAGGED_MODES)}"
    tensors = list(tensors)
    assert len(tensors) > 0 or out is not None, "an empty list needs an output table to tell width, dtype and device"
    first = tensors[0] if tensors else out
    dtype, dev = first.dtype, first.device
    assert dtype in ELEM_DTYPE_CODES, f"unsupported dtype {dtype} (float32, float16, bfloat16)"
    d = int(first.shape[1]) if tensors else int(out.shape[1])
    # shapes and dtypes first, then the devices: every refusal comes before the library is touched
    for i, t in enumerate(tensors):
        assert isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == d and t.dtype == dtype, \
            f"tensor {i}: every tensor must be (rows, {d}) of {dtype}"
    desc = np.empty((len(tensors) + 1, 5), np.int64)  # rows 0 .. n-1: pointer, rows, strides, start; row n: the total
    total = 0
    for i, t in enumerate(tensors):
        assert t.is_cuda and t.device == dev, f"tensor {i}: every tensor must be on one GPU"
        desc[i] = (t.data_ptr(), t.shape[0], t.stride(0), t.stride(1), total)
        total += int(t.shape[0])
    desc[len(tensors)] = (0, 0, 0, 0, total)
    if out is None:
        out = torch.empty((total, d), dtype=dtype, device=dev)
    assert out.is_cuda and out.device == dev and out.dtype == dtype and out.dim() == 2 and out.shape[0] == total and \
        out.shape[1] >= d and (out.shape[1] <= 1 or out.stride(1) == 1) and (total <= 1 or out.stride(0) >= out.shape[1]), \
        f"the output must be a row-major ({total}, >= {d}) table of {dtype} on the tensors' device"
    require_gpu()
    seg = torch.empty(total, dtype=torch.int32, device=dev) if return_segments else None
    if total > 0 and d > 0:
        n = len(tensors)
        # one upload: [n, 4] descriptors followed by the n + 1 prefix sums
        packed = np.concatenate([desc[:n, :4].reshape(-1), desc[:, 4]])
        up = torch.from_numpy(packed).to(dev, non_blocking=False)
        ld = int(out.stride(0)) if total > 1 else max(int(out.stride(0)), int(out.shape[1]))
        launch("runia_ragged_rows", up.data_ptr(), up.data_ptr() + 32 * n, n, total, d, ELEM_DTYPE_CODES[dtype],
               _RAGGED_MODES[mode], out.data_ptr(), ld, _ptr(seg))
    return (out, seg) if return_segments else out


def _kl_samples(z: torch.Tensor, n_mc: int):
    """Prologue of the kl_entropy wrappers: the GPU first, then z [N*n_mc, D] f32 on it -> ``(z contiguous, N, D)``."""
    require_gpu()
    assert z.is_cuda and z.dtype == torch.float32 and z.dim() == 2
    return z.contiguous(), z.shape[0] // n_mc, z.shape[1]


@_device_guard()
def kl_entropy_per_dim(z: torch.Tensor, n_mc: int, k: int, min_dist: float = 1e-5) -> torch.Tensor:
    """z [N*n_mc, D] f32 -> h [N, D] f64."""
    z, n, d = _kl_samples(z, n_mc)
    h = torch.empty((n, d), dtype=torch.float64, device=z.device)
    launch("runia_kl_entropy_per_dim_f32", z.data_ptr(), h.data_ptr(), n, n_mc, d, k, min_dist)
    return h


@_device_guard()
def kl_entropy_joint(z: torch.Tensor, n_mc: int, k: int, min_dist: float = 1e-5) -> torch.Tensor:
    """z [N*n_mc, D] f32 -> h_mvn [N] f64."""
    z, n, d = _kl_samples(z, n_mc)
    h = torch.empty((n,), dtype=torch.float64, device=z.device)
    launch("runia_kl_entropy_joint_f32", z.data_ptr(), h.data_ptr(), n, n_mc, d, k, min_dist)
    return h


@_device_guard()
def kl_entropy_both(z: torch.Tensor, n_mc: int, k: int, min_dist: float = 1e-5):
    """z [N*n_mc, D] f32 -> (h_mvn [N] f64, h [N, D] f64): both outputs of ``get_dl_h_z`` from one read of the samples
    (``runia_kl_entropy_both_f32``; same bits as :func:`kl_entropy_joint` and :func:`kl_entropy_per_dim`)."""
    z, n, d = _kl_samples(z, n_mc)
    h_mvn = torch.empty((n,), dtype=torch.float64, device=z.device)
    h = torch.empty((n, d), dtype=torch.float64, device=z.device)
    launch("runia_kl_entropy_both_f32", z.data_ptr(), h_mvn.data_ptr(), h.data_ptr(), n, n_mc, d, k, min_dist)
    return h_mvn, h


@_device_guard()
def pack_weights(b: torch.Tensor) -> torch.Tensor:
    """B [K, n] f64 (device) -> fragment-ordered copy for the f64 MFMA kernels."""
    require_gpu()
    assert b.is_cuda and b.dtype == torch.float64 and b.dim() == 2
    b = b.contiguous()
    k, n = b.shape
    packed = torch.empty((query("runia_packed_weights_bytes", k, n) // 8,), dtype=torch.float64, device=b.device)
    launch("runia_pack_weights_f64", b.data_ptr(), n, k, n, packed.data_ptr())
    return packed


@_device_guard()
def pca_transform(x: torch.Tensor, packed_ct: torch.Tensor, bias: torch.Tensor, scale: Optional[torch.Tensor], n: int) -> torch.Tensor:
    """x [N, D] f64/f32 -> y [N, n] f64."""
    require_gpu()
    assert x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64)
    x = x.contiguous()
    nrow, d = x.shape
    y = torch.empty((nrow, n), dtype=torch.float64, device=x.device)
    launch("runia_pca_transform_f32in" if x.dtype == torch.float32 else "runia_pca_transform_f64", x.data_ptr(),
           packed_ct.data_ptr(), bias.data_ptr(), _ptr(scale), y.data_ptr(), nrow, d, n, 0 if scale is None else 1)
    return y


@_device_guard()
def md_score(x: torch.Tensor, mean: torch.Tensor, packed_p: torch.Tensor, *, _family: str = "runia_md_score_ws") -> torch.Tensor:
    """x [N, n] (f64 or f32), mean [n] (f64 or f32) -> score [N] f64 = -(x-mean) P (x-mean)^T,
    with ``x - mean`` formed under NumPy's dtype rules (f32 only when both are f32).  (``_family``: the entry points' common
    prefix; ``md_score_tril`` is this body on ``runia_md_score_tril_*``.)"""
    lib = load_library()
    require_gpu()
    assert x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64)
    x = x.contiguous()
    nrow, n = x.shape
    if x.dtype == torch.float64:
        mean = mean.to(torch.float64)
        name = _family + "_f64"
    elif mean.dtype == torch.float32:
        name = _family + "_f32"
    else:
        mean = mean.to(torch.float64)
        name = _family + "_f32x_f64mean"
    mean = mean.contiguous()
    s = torch.empty((nrow,), dtype=torch.float64, device=x.device)
    # few rows of wide features: column blocks on separate workgroups + a replay launch (same bits, see runia_hip.h)
    ws_bytes = int(lib.runia_md_score_workspace_bytes(nrow, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    launch(name, x.data_ptr(), mean.data_ptr(), packed_p.data_ptr(), s.data_ptr(), _ptr(ws), ws_bytes, nrow, n)
    return s


def md_score_tril(x: torch.Tensor, mean: torch.Tensor, packed_wt: torch.Tensor) -> torch.Tensor:
    """``md_score`` from the triangular factor of the precision (``runia_md_score_tril_*``): precision = W^T W with W lower
    triangular, ``packed_wt = pack_weights(W^T)``; score [N] f64 = -|| W (x - mean) ||^2, same centring rules as ``md_score``."""
    return md_score(x, mean, packed_wt, _family="runia_md_score_tril")


@_device_guard()
def mahalanobis_score(x: torch.Tensor, class_mean: torch.Tensor, packed_p: torch.Tensor, mu_p: torch.Tensor,
                      class_loop: bool = False, split: bool = True) -> torch.Tensor:
    """x [N, D], class_mean [C, D] (both f32 or both f64) -> score [N] f64.  ``class_loop=True`` hands over the small
    workspace only (more than 16 classes then take the per-class loop instead of the matrix-core form; tests).
    ``split=False`` (up to 16 classes; tests and measurements) hands over NO workspace: the entry point then keeps the
    one-launch form instead of the column-split launches - the same bits."""
    require_gpu()
    assert x.is_cuda and x.dim() == 2 and x.dtype == class_mean.dtype
    x = x.contiguous()
    class_mean = class_mean.contiguous()
    nrow, d = x.shape
    c = class_mean.shape[0]
    s = torch.empty((nrow,), dtype=torch.float64, device=x.device)
    ws_bytes = (query("runia_mahalanobis_workspace_bytes", nrow, d) if class_loop
                else query("runia_mahalanobis_workspace_bytes_classes", nrow, d, c))
    ws = workspace(ws_bytes, x.device, 8)
    no_ws = (not split) and c <= 16
    launch("runia_mahalanobis_score_f32" if x.dtype == torch.float32 else "runia_mahalanobis_score_f64", x.data_ptr(),
           class_mean.data_ptr(), packed_p.data_ptr(), mu_p.data_ptr(), s.data_ptr(), None if no_ws else ws.data_ptr(),
           0 if no_ws else ws_bytes, nrow, d, c)
    return s


@_device_guard()
def row_lse_msp(logits: torch.Tensor, want_lse: bool = True, want_msp: bool = False):
    """logits [N, C] f32 -> (lse [N] f32 | None, msp [N] f32 | None)."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    logits = logits.contiguous()
    n, c = logits.shape
    lse = torch.empty((n,), dtype=torch.float32, device=logits.device) if want_lse else None
    msp = torch.empty((n,), dtype=torch.float32, device=logits.device) if want_msp else None
    launch("runia_row_lse_msp_f32", logits.data_ptr(), _ptr(lse), _ptr(msp), n, c)
    return lse, msp


class LogitRowStats(NamedTuple):
    """What ``logit_row_stats`` returns: [N] device tensors, ``None`` for a statistic that was not asked for."""

    max_logit: Optional[torch.Tensor]
    lse: Optional[torch.Tensor]
    neg_entropy: Optional[torch.Tensor]
    argmax: Optional[torch.Tensor]


@_device_guard()
def logit_row_stats(logits: torch.Tensor, max_logit: bool = True, lse: bool = True, neg_entropy: bool = True,
                    argmax: bool = True) -> LogitRowStats:
    """logits [N, C] f32 -> row maximum, logsumexp, ``sum p log p`` of the softmax (f32) and the first argmax (int32) in
    one pass (``runia_row_logit_stats_f32``); at least one statistic must be asked for."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    assert max_logit or lse or neg_entropy or argmax, "ask for at least one statistic"
    logits = logits.contiguous()
    n, c = logits.shape
    f32 = lambda want: torch.empty((n,), dtype=torch.float32, device=logits.device) if want else None  # noqa: E731
    out = LogitRowStats(f32(max_logit), f32(lse), f32(neg_entropy),
                        torch.empty((n,), dtype=torch.int32, device=logits.device) if argmax else None)
    launch("runia_row_logit_stats_f32", logits.data_ptr(), _ptr(out.max_logit), _ptr(out.lse), _ptr(out.neg_entropy),
           _ptr(out.argmax), n, c)
    return out


@_device_guard()
def klm_score(logits: torch.Tensor, lse: torch.Tensor, neg_entropy: torch.Tensor, log_q: torch.Tensor,
              valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``max_c sum_k softmax(logits)[n, k] log_q[c, k] - neg_entropy[n]`` over the classes with ``valid[c] != 0`` -> [N] f32
    (``runia_klm_score_f32``).  logits [N, C], log_q [K, C] f32; lse, neg_entropy [N] f32 from ``logit_row_stats``; valid [K]
    int32 or None."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    assert log_q.is_cuda and log_q.dtype == torch.float32 and log_q.dim() == 2 and log_q.shape[1] == logits.shape[1]
    n, c = logits.shape
    k = log_q.shape[0]
    assert lse.dtype == torch.float32 and neg_entropy.dtype == torch.float32 and lse.shape == (n,) and neg_entropy.shape == (n,)
    assert valid is None or (valid.is_cuda and valid.dtype == torch.int32 and valid.shape == (k,))
    logits, log_q = logits.contiguous(), log_q.contiguous()
    lse, neg_entropy = lse.contiguous(), neg_entropy.contiguous()
    valid = None if valid is None else valid.contiguous()
    score = torch.empty((n,), dtype=torch.float32, device=logits.device)
    launch("runia_klm_score_f32", logits.data_ptr(), lse.data_ptr(), neg_entropy.data_ptr(), log_q.data_ptr(), _ptr(valid),
           score.data_ptr(), n, c, k)
    return score


@_device_guard()
def fdbd_score(logits: torch.Tensor, inv_dist: torch.Tensor, feat_dist: torch.Tensor) -> torch.Tensor:
    """logits [N, C], inv_dist [C, C], feat_dist [N], all f32 -> [N] f32 (``runia_fdbd_score_f32``); C >= 2."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    n, c = logits.shape
    assert c >= 2, "fDBD needs at least two classes"
    assert inv_dist.is_cuda and inv_dist.dtype == torch.float32 and inv_dist.shape == (c, c)
    assert feat_dist.is_cuda and feat_dist.dtype == torch.float32 and feat_dist.shape == (n,)
    logits, inv_dist, feat_dist = logits.contiguous(), inv_dist.contiguous(), feat_dist.contiguous()
    score = torch.empty((n,), dtype=torch.float32, device=logits.device)
    launch("runia_fdbd_score_f32", logits.data_ptr(), inv_dist.data_ptr(), feat_dist.data_ptr(), score.data_ptr(), n, c)
    return score


@_device_guard()
def row_dist(x: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
    """``|| x[n] - mu ||_2`` -> [N] f32 (x [N, D], mu [D], f32; ``runia_row_dist_f32``)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    assert mu.is_cuda and mu.dtype == torch.float32 and mu.numel() == x.shape[1]
    x, mu = x.contiguous(), mu.contiguous()
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    launch("runia_row_dist_f32", x.data_ptr(), mu.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1])
    return out


class CalibrationRows(NamedTuple):
    """What ``calibration_rows`` returns: [N] device tensors (``pred`` int32, the rest float32), ``None`` where not asked for."""

    pred: Optional[torch.Tensor]
    conf: Optional[torch.Tensor]
    nll: Optional[torch.Tensor]
    brier: Optional[torch.Tensor]
    g: Optional[torch.Tensor]
    h: Optional[torch.Tensor]


def _calib_labels(labels: Optional[torch.Tensor], n: int, ignore_index: Optional[int]):
    """-> (labels contiguous | None, is-int64 flag, has-ignore flag, ignore value) as the calibration entry points take them."""
    if labels is not None:
        assert labels.is_cuda and labels.dtype in (torch.int32, torch.int64) and labels.shape == (n,)
        labels = labels.contiguous()
    return (labels, int(labels is not None and labels.dtype == torch.int64), int(ignore_index is not None),
            0 if ignore_index is None else int(ignore_index))


@_device_guard()
def calibration_rows(logits: torch.Tensor, labels: Optional[torch.Tensor], beta: float = 1.0, ignore_index: Optional[int] = None,
                     want=("pred", "conf", "nll", "brier", "g", "h")) -> CalibrationRows:
    """One read of logits [N, C] (f32 / f16 / bf16, read where they lie) at the temperature ``1 / beta`` -> the per-row outputs
    named in ``want`` (``runia_calib_rows``).  labels [N] int32 / int64, or None (``pred`` and ``conf`` only).  A row whose label is
    ``ignore_index`` or outside ``[0, C)`` gets ``pred`` and NaN elsewhere; callers validate labels."""
    require_gpu()
    assert logits.is_cuda and logits.dim() == 2 and logits.dtype in ELEM_DTYPE_CODES, \
        f"logits: a [N, C] device tensor of float32, float16 or bfloat16, got {tuple(logits.shape)} {logits.dtype}"
    names = CalibrationRows._fields
    assert want and set(want) <= set(names), f"want: a non-empty subset of {names}"
    assert labels is not None or set(want) <= {"pred", "conf"}, "nll, brier, g and h need labels"
    logits = logits.contiguous()
    n, c = logits.shape
    labels, is64, has_ignore, ignore = _calib_labels(labels, n, ignore_index)
    out = CalibrationRows(*(torch.empty((n,), dtype=torch.int32 if k == "pred" else torch.float32, device=logits.device)
                            if k in want else None for k in names))
    launch("runia_calib_rows", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], _ptr(labels), is64, has_ignore, ignore,
           float(beta), *(_ptr(t) for t in out), n, c)
    return out


@_device_guard()
def calibration_reduce(rows: CalibrationRows, labels: torch.Tensor, n_bins: int, ignore_index: Optional[int] = None) -> torch.Tensor:
    """The per-row table -> the device record of ``runia_calib_reduce_f32``: int64 [6 + 3 n_bins] whose slots 2..5 and the last
    ``n_bins`` hold float64 bits (``calibration_record`` splits a host copy).  Fixed summation order: the same bits every run."""
    require_gpu()
    n = labels.shape[0]
    assert 0 <= n_bins <= 512, "n_bins: 0 .. 512"
    assert n_bins == 0 or rows.conf is not None, "the reliability table needs conf"
    assert all(t is None or (t.is_cuda and t.shape == (n,) and t.is_contiguous()) for t in rows)
    labels, is64, has_ignore, ignore = _calib_labels(labels, n, ignore_index)
    out = torch.empty((6 + 3 * n_bins,), dtype=torch.int64, device=labels.device)
    ws_bytes = query("runia_calib_reduce_workspace_bytes", n, n_bins)
    ws = workspace(ws_bytes, labels.device)
    launch("runia_calib_reduce_f32", _ptr(rows.pred), _ptr(rows.conf), _ptr(rows.nll), _ptr(rows.brier), _ptr(rows.g), _ptr(rows.h),
           labels.data_ptr(), is64, has_ignore, ignore, n, n_bins, out.data_ptr(), ws.data_ptr(), ws_bytes)
    return out


def calibration_record(record: np.ndarray, n_bins: int) -> dict:
    """A host copy of ``calibration_reduce``'s record -> its named parts (ints and float64 arrays)."""
    f = record.view(np.float64)
    return {"n_used": int(record[0]), "n_correct": int(record[1]), "nll": float(f[2]), "brier": float(f[3]), "g": float(f[4]),
            "h": float(f[5]), "count": record[6:6 + n_bins].copy(), "correct": record[6 + n_bins:6 + 2 * n_bins].copy(),
            "conf_sum": f[6 + 2 * n_bins:6 + 3 * n_bins].copy()}


PIXCAL_MODES = {m: _HEADER_MACROS["RUNIA_PIXCAL_MODE_" + m.upper()] for m in ("head", "top", "classwise")}
PIXCAL_HEAD_SLOTS = _HEADER_MACROS["RUNIA_PIXCAL_HEAD_SLOTS"]
PIXCAL_MAX_BINS = _HEADER_MACROS["RUNIA_PIXCAL_MAX_BINS"]
PIXCAL_MAX_CLASSES = _HEADER_MACROS["RUNIA_PIXCAL_MAX_CLASSES"]
PIXCAL_MAX_CLASSWISE = _HEADER_MACROS["RUNIA_PIXCAL_MAX_CLASSWISE"]  # C * n_bins of the class-wise table
PIXCAL_MAX_PIXELS = 1 << 34
# label dtype of the (G, H, W) masks -> the `label_dtype` code of runia_pixel_calib_accumulate
PIXCAL_LABEL_CODES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}


def pixel_calibration_record_slots(c: int, n_bins: int, classwise: bool) -> int:
    """8-byte slots of the record of ``runia_pixel_calib_accumulate`` for ``c`` classes and ``n_bins`` bins."""
    return PIXCAL_HEAD_SLOTS + 3 * n_bins + 3 * c + (3 * c * n_bins if classwise else 0)


@_device_guard()
def pixel_calibration_accumulate(logits: torch.Tensor, labels: Optional[torch.Tensor], record: Optional[torch.Tensor],
                                 beta: float = 1.0, n_bins: int = 15, mode: str = "top", ignore_index: Optional[int] = None,
                                 conf_map: Optional[torch.Tensor] = None, pred_map: Optional[torch.Tensor] = None) -> None:
    """One pass over ``logits`` (G, C, H, W) (f32 / f16 / bf16 on the device, any strides, read in place) against ``labels``
    (G, H, W) int64 / int32 / uint8 that ADDS into ``record`` (int64 device tensor the caller zeroed, at least
    ``pixel_calibration_record_slots`` long; ``pixel_calibration_record`` splits a host copy) - ``runia_pixel_calib_accumulate``.
    ``mode``: ``"head"`` (``n_bins`` is not used), ``"top"`` or ``"classwise"``.  ``conf_map`` f32 / ``pred_map`` int32
    (G, H, W) contiguous are filled for every pixel when given.  Stream-ordered; nothing is read back."""
    assert logits.is_cuda and logits.dim() == 4 and logits.dtype in ELEM_DTYPE_CODES, \
        f"logits: a (G, C, H, W) device tensor of float32, float16 or bfloat16, got {tuple(logits.shape)} {logits.dtype}"
    assert mode in PIXCAL_MODES, f"mode must be one of {tuple(PIXCAL_MODES)}"
    g, c, h, w = (int(v) for v in logits.shape)
    n_bins = 0 if mode == "head" else int(n_bins)
    assert record is not None or conf_map is not None or pred_map is not None
    if record is not None:
        assert labels is not None and labels.is_cuda and labels.dtype in PIXCAL_LABEL_CODES and tuple(labels.shape) == (g, h, w), \
            f"labels: a (G, H, W) device tensor of int64, int32 or uint8 matching the logits, got {labels.dtype}"
        labels = labels.contiguous()
        need = PIXCAL_HEAD_SLOTS if mode == "head" else pixel_calibration_record_slots(c, n_bins, mode == "classwise")
        assert record.is_cuda and record.dtype == torch.int64 and record.is_contiguous() and record.numel() >= need
    for t, dt in ((conf_map, torch.float32), (pred_map, torch.int32)):
        assert t is None or (t.is_cuda and t.dtype == dt and tuple(t.shape) == (g, h, w) and t.is_contiguous())
    require_gpu()
    if g == 0 or h * w == 0:
        return
    ws_bytes = query("runia_pixel_calib_workspace_bytes", g, c, h, w, n_bins, PIXCAL_MODES[mode])
    ws = workspace(ws_bytes, logits.device)
    sn, sc, sh, sw = (int(v) for v in logits.stride())
    launch("runia_pixel_calib_accumulate", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], g, c, h, w, sn, sc, sh, sw,
           _ptr(labels) if record is not None else None, PIXCAL_LABEL_CODES[labels.dtype] if record is not None else 0,
           int(ignore_index is not None), 0 if ignore_index is None else int(ignore_index), float(beta), n_bins,
           PIXCAL_MODES[mode], _ptr(record), _ptr(conf_map), _ptr(pred_map), ws.data_ptr(), ws_bytes)


def pixel_calibration_record(record: np.ndarray, c: int, n_bins: int, classwise: bool) -> dict:
    """A host copy of the record of ``pixel_calibration_accumulate`` -> its named parts (ints, float64 and int64 arrays).
    ``n_bins = 0``: the head alone."""
    record = np.ascontiguousarray(record, dtype=np.int64)
    f = record.view(np.float64)
    out = {"n_used": int(record[0]), "n_correct": int(record[1]), "n_bad": int(record[2]), "nll": float(f[3]),
           "brier": float(f[4]), "g": float(f[5]), "h": float(f[6])}
    if n_bins == 0:
        return out
    o = PIXCAL_HEAD_SLOTS
    out.update(count=record[o:o + n_bins].copy(), correct=record[o + n_bins:o + 2 * n_bins].copy(),
               conf_sum=f[o + 2 * n_bins:o + 3 * n_bins].copy())
    o += 3 * n_bins
    out.update(support=record[o:o + c].copy(), predicted=record[o + c:o + 2 * c].copy(), hit=record[o + 2 * c:o + 3 * c].copy())
    o += 3 * c
    if classwise:
        e = c * n_bins
        out.update(cw_count=record[o:o + e].reshape(c, n_bins).copy(), cw_pos=record[o + e:o + 2 * e].reshape(c, n_bins).copy(),
                   cw_conf_sum=f[o + 2 * e:o + 3 * e].reshape(c, n_bins).copy())
    return out


PIXSML_HEAD_SLOTS = _HEADER_MACROS["RUNIA_PIXSML_HEAD_SLOTS"]
PIXSML_MAX_CLASSES = _HEADER_MACROS["RUNIA_PIXSML_MAX_CLASSES"]
PIXSML_TILE = (_HEADER_MACROS["RUNIA_PIXSML_TILE_H"], _HEADER_MACROS["RUNIA_PIXSML_TILE_W"])
PIXSML_MAX_WIDTH = _HEADER_MACROS["RUNIA_PIXSML_MAX_WIDTH"]
PIXSML_MAX_DILATION = _HEADER_MACROS["RUNIA_PIXSML_MAX_DILATION"]
PIXSML_KERNEL_SIZES = (3, 5, 7)
PIXSML_MAX_PIXELS = 1 << 34   # of one call, and of one record over all its calls
PIXSML_Q_BITS = 16            # a used max logit enters the record as rint(m * 2^16)


def pixel_sml_record_slots(c: int) -> int:
    """8-byte slots of the record of ``runia_pixel_sml_accumulate`` for ``c`` classes."""
    return PIXSML_HEAD_SLOTS + 4 * c


def _logits_view(logits: torch.Tensor):
    assert logits.is_cuda and logits.dim() == 4 and logits.dtype in ELEM_DTYPE_CODES, \
        f"logits: a (G, C, H, W) device tensor of float32, float16 or bfloat16, got {tuple(logits.shape)} {logits.dtype}"
    return tuple(int(v) for v in logits.shape), tuple(int(v) for v in logits.stride())


@_device_guard()
def pixel_sml_accumulate(logits: torch.Tensor, record: torch.Tensor, valid: Optional[torch.Tensor] = None) -> None:
    """One pass over ``logits`` (G, C, H, W) (f32 / f16 / bf16 on the device, any strides, read in place) that ADDS the integer
    moments of every pixel's max logit, by predicted class, into ``record`` (int64 device tensor the caller zeroed, at least
    ``pixel_sml_record_slots(C)`` long; ``pixel_sml_record`` splits a host copy) - ``runia_pixel_sml_accumulate``.  ``valid``:
    bool / uint8 (G, H, W) or None (every pixel).  Stream-ordered; nothing is read back."""
    (g, c, h, w), (sn, sc, sh, sw) = _logits_view(logits)
    assert record.is_cuda and record.dtype == torch.int64 and record.is_contiguous() and \
        record.numel() >= pixel_sml_record_slots(c), f"record: an int64 device tensor of at least {pixel_sml_record_slots(c)} slots"
    if valid is not None:
        assert valid.is_cuda and valid.dtype in (torch.bool, torch.uint8) and tuple(valid.shape) == (g, h, w), \
            f"valid: a (G, H, W) device tensor of bool or uint8 matching the logits, got {tuple(valid.shape)} {valid.dtype}"
        valid = valid.contiguous()
    require_gpu()
    if g == 0 or h * w == 0:
        return
    launch("runia_pixel_sml_accumulate", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], g, c, h, w, sn, sc, sh, sw,
           _ptr(valid), record.data_ptr())


def pixel_sml_record(record: np.ndarray, c: int) -> dict:
    """A host copy of the record of ``pixel_sml_accumulate`` -> its named parts: Python ints and lists of Python ints
    (``sumsq = sq_hi * 2^30 + sq_lo`` put together exactly)."""
    record = np.ascontiguousarray(record, dtype=np.int64)
    u = record.view(np.uint64)
    o = PIXSML_HEAD_SLOTS
    return {"n_used": int(record[0]), "n_masked": int(record[1]), "n_bad": int(record[2]),
            "count": [int(v) for v in record[o:o + c]], "sum_q": [int(v) for v in record[o + c:o + 2 * c]],
            "sumsq": [(int(hi) << 30) + int(lo) for hi, lo in zip(u[o + 2 * c:o + 3 * c], u[o + 3 * c:o + 4 * c])]}


@_device_guard()
def pixel_sml_maps(logits: torch.Tensor, mean: torch.Tensor, inv_std: torch.Tensor, want_max_logit: bool = False) -> dict:
    """``{"sml": f32, "label": int32[, "max_logit": f32]}`` (G, H, W) of ``logits`` (G, C, H, W) read in place: ``sml = (m -
    mean[label]) * inv_std[label]`` with ``m``, ``label`` the max and argmax over the classes - ``runia_pixel_sml_maps``, one
    launch.  ``mean``, ``inv_std``: f32 [C] on the device."""
    (g, c, h, w), (sn, sc, sh, sw) = _logits_view(logits)
    for name, t in (("mean", mean), ("inv_std", inv_std)):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (c,) and t.is_contiguous(), \
            f"{name}: a contiguous float32 device tensor of {c} entries, got {tuple(t.shape)} {t.dtype}"
    dev = logits.device
    out = {"sml": torch.empty((g, h, w), dtype=torch.float32, device=dev),
           "label": torch.empty((g, h, w), dtype=torch.int32, device=dev)}
    if want_max_logit:
        out["max_logit"] = torch.empty((g, h, w), dtype=torch.float32, device=dev)
    require_gpu()
    if g == 0 or h * w == 0:
        return out
    launch("runia_pixel_sml_maps", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], g, c, h, w, sn, sc, sh, sw,
           mean.data_ptr(), inv_std.data_ptr(), out["sml"].data_ptr(), out["label"].data_ptr(), _ptr(out.get("max_logit")))
    return out


def gaussian_taps(kernel_size: int, sigma: float) -> np.ndarray:
    """The ``kernel_size`` taps ``exp(-(a - (K - 1) / 2)^2 / (2 sigma^2))`` in float64, normalised to sum 1, rounded to f32."""
    a = np.arange(kernel_size, dtype=np.float64) - (kernel_size - 1) / 2.0
    g = np.exp(-(a * a) / (2.0 * float(sigma) * float(sigma)))
    return np.ascontiguousarray((g / g.sum()).astype(np.float32))


@_device_guard()
def pixel_boundary_smooth(score: torch.Tensor, label: Optional[torch.Tensor], boundary_width: int = 4,
                          boundary_iterations: int = 4, taps: Optional[np.ndarray] = None, dilation: int = 6) -> torch.Tensor:
    """Boundary suppression (skipped when ``boundary_width`` or ``boundary_iterations`` is 0), then the dilated Gaussian smoothing
    with the host f32 ``taps`` (3, 5 or 7 of them; None: skipped) of a contiguous f32 (G, H, W) device map, per image, with
    clamped coordinates at the image border - ``runia_pixel_boundary_smooth_f32``.  ``label``: int32 (G, H, W), needed by the
    suppression.  Returns a new map."""
    assert score.is_cuda and score.dim() == 3 and score.dtype == torch.float32 and score.is_contiguous(), \
        f"score: a contiguous float32 (G, H, W) device tensor, got {tuple(score.shape)} {score.dtype}"
    g, h, w = (int(v) for v in score.shape)
    wb, it = int(boundary_width), int(boundary_iterations)
    suppress = wb > 0 and it > 0
    assert 0 <= wb <= PIXSML_MAX_WIDTH and 0 <= it <= PIXSML_MAX_WIDTH and (not suppress or wb % it == 0), \
        f"boundary_width {wb} / boundary_iterations {it}: 0 .. {PIXSML_MAX_WIDTH}, the width a multiple of the iterations"
    if suppress:
        assert label is not None and label.is_cuda and label.dtype == torch.int32 and tuple(label.shape) == (g, h, w) and \
            label.is_contiguous(), "label: a contiguous int32 (G, H, W) device tensor matching the score map"
    k = 0
    if taps is not None:
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        k = int(taps.size)
        assert taps.ndim == 1 and k in PIXSML_KERNEL_SIZES and 1 <= int(dilation) <= PIXSML_MAX_DILATION, \
            f"{k} taps at dilation {dilation}: 3, 5 or 7 taps, dilation 1 .. {PIXSML_MAX_DILATION}"
    require_gpu()
    out = torch.empty_like(score)
    if g == 0 or h * w == 0:
        return out
    ws_bytes = query("runia_pixel_boundary_smooth_workspace_bytes", g, h, w, wb, it, k)
    ws = workspace(ws_bytes, score.device)
    launch("runia_pixel_boundary_smooth_f32", score.data_ptr(), _ptr(label) if suppress else None, g, h, w, wb, it, k,
           int(dilation) if k else 0, taps.ctypes.data if k else None, out.data_ptr(), ws.data_ptr(), ws_bytes)
    return out


MASKQ_MAX_CLASSES = _HEADER_MACROS["RUNIA_MASKQ_MAX_CLASSES"]
MASKQ_MAX_QUERIES = _HEADER_MACROS["RUNIA_MASKQ_MAX_QUERIES"]
MASKQ_MAX_SIDE = _HEADER_MACROS["RUNIA_MASKQ_MAX_SIDE"]
MASKQ_MAX_PIXELS = 1 << _HEADER_MACROS["RUNIA_MASKQ_MAX_PIXELS_LOG2"]
MASKQ_MAX_PLANE_SPAN = (1 << 31) - 1   # (h - 1) sh + (w - 1) sw of the mask logits: the tap offsets are 32-bit
MASKQ_OUTPUTS = ("rba", "max_score", "label", "eam", "semseg")


@_device_guard()
def maskq_maps(class_logits: torch.Tensor, mask_logits: torch.Tensor, size=None, outputs=("rba",),
               has_void: bool = True) -> dict:
    """The maps ``outputs`` (of ``MASKQ_OUTPUTS``) of a mask classifier's ``class_logits`` (G, Q, K + 1; (G, Q, K) without
    ``has_void``) and ``mask_logits`` (G, Q, h, w), both f32 / f16 / bf16 device tensors read in place through their strides,
    upsampled to ``size`` = (H, W) (None: (h, w)) - ``runia_maskq_maps``, two launches.  f32 (G, H, W) each, ``label`` int32,
    ``semseg`` f32 (G, K, H, W)."""
    for name, t, nd in (("class_logits", class_logits, 3), ("mask_logits", mask_logits, 4)):
        assert t.is_cuda and t.dim() == nd and t.dtype in ELEM_DTYPE_CODES, \
            f"{name}: a {nd}-dimensional device tensor of float32, float16 or bfloat16, got {tuple(t.shape)} {t.dtype}"
    g, q, h, w = (int(v) for v in mask_logits.shape)
    k = int(class_logits.shape[2]) - (1 if has_void else 0)
    assert tuple(class_logits.shape[:2]) == (g, q) and 1 <= k <= MASKQ_MAX_CLASSES and 1 <= q <= MASKQ_MAX_QUERIES, \
        f"class_logits {tuple(class_logits.shape)} against mask_logits {tuple(mask_logits.shape)}: the same G and Q, " \
        f"1 .. {MASKQ_MAX_CLASSES} classes, 1 .. {MASKQ_MAX_QUERIES} queries"
    big_h, big_w = (h, w) if size is None else (int(size[0]), int(size[1]))
    names = tuple(outputs)
    assert names and all(n in MASKQ_OUTPUTS for n in names), f"outputs: some of {MASKQ_OUTPUTS}, got {names}"
    assert (h * w > 0 or big_h * big_w == 0) and 0 <= big_h <= MASKQ_MAX_SIDE and 0 <= big_w <= MASKQ_MAX_SIDE and \
        g * big_h * big_w <= MASKQ_MAX_PIXELS, f"size {(big_h, big_w)} of {g} images from {(h, w)}"
    dev = mask_logits.device
    out = {n: torch.empty((g, k, big_h, big_w) if n == "semseg" else (g, big_h, big_w),
                          dtype=torch.int32 if n == "label" else torch.float32, device=dev) for n in names}
    require_gpu()
    if g == 0 or big_h * big_w == 0:
        return out
    cg, cq, ck = (int(v) for v in class_logits.stride())
    sn, sc, sh, sw = (int(v) for v in mask_logits.stride())
    ws_bytes = query("runia_maskq_workspace_bytes", g, q, k, big_h, big_w, h, w)
    ws = workspace(ws_bytes, dev)
    launch("runia_maskq_maps", class_logits.data_ptr(), ELEM_DTYPE_CODES[class_logits.dtype], cg, cq, ck, 1 if has_void else 0,
           mask_logits.data_ptr(), ELEM_DTYPE_CODES[mask_logits.dtype], g, q, k, h, w, sn, sc, sh, sw, big_h, big_w,
           _ptr(out.get("rba")), _ptr(out.get("max_score")), _ptr(out.get("label")), _ptr(out.get("eam")),
           _ptr(out.get("semseg")), ws.data_ptr(), ws_bytes)
    return out


CONFORMAL_METHODS = {"lac": 0, "aps": 1, "raps": 2}  # `method` of the runia_conformal_* entry points


class ConformalSets(NamedTuple):
    """What ``conformal_sets`` returns: ``size`` [N] int32, ``members`` [N, ceil(C / 32)] int32 (bit ``c % 32`` of word ``c // 32``
    is class ``c``) or None, ``covered`` [N] uint8 or None (no labels)."""

    size: torch.Tensor
    members: Optional[torch.Tensor]
    covered: Optional[torch.Tensor]


def conformal_max_classes() -> int:
    """The widest row ``conformal_sets`` orders (``runia_conformal_max_classes``)."""
    return query("runia_conformal_max_classes")


def _conformal_rows(logits: torch.Tensor, u: Optional[torch.Tensor], method: str):
    """Checks shared by the two conformal row kernels -> (logits with unit column stride, u contiguous | None, method code)."""
    assert logits.is_cuda and logits.dim() == 2 and logits.shape[1] >= 1 and logits.dtype in ELEM_DTYPE_CODES, \
        f"logits: a [N, C] device tensor of float32, float16 or bfloat16, got {tuple(logits.shape)} {logits.dtype}"
    assert method in CONFORMAL_METHODS, f"method: one of {tuple(CONFORMAL_METHODS)}, got {method!r}"
    n, c = logits.shape
    if (c > 1 and logits.stride(1) != 1) or (n > 1 and logits.stride(0) < c):  # (row-sliced views are read where they lie)
        logits = logits.contiguous()
    if u is not None:
        assert u.is_cuda and u.dtype == torch.float32 and u.shape == (n,), "u: a [N] float32 device tensor"
        u = u.contiguous()
    return logits, u, CONFORMAL_METHODS[method]


@_device_guard()
def conformal_label_scores(logits: torch.Tensor, labels: torch.Tensor, method: str = "aps", beta: float = 1.0,
                           u: Optional[torch.Tensor] = None, lam: float = 0.0, k_reg: int = 0,
                           ignore_index: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The conformal score ``s_y`` (float32) and the 1-based rank ``r_y`` (int32) of every row's label from one read of logits
    [N, C] at the temperature ``1 / beta`` (``runia_conformal_label_scores``).  ``u`` [N] float32 or None (u = 1).  A row whose
    label is ``ignore_index`` or outside ``[0, C)``, and a row without a softmax, gets NaN and rank 0."""
    require_gpu()
    logits, u, code = _conformal_rows(logits, u, method)
    n, c = logits.shape
    labels, is64, has_ignore, ignore = _calib_labels(labels, n, ignore_index)
    assert labels is not None, "the label scores need labels"
    score = torch.empty((n,), dtype=torch.float32, device=logits.device)
    rank = torch.empty((n,), dtype=torch.int32, device=logits.device)
    launch("runia_conformal_label_scores", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], logits.stride(0) if n > 1 else c,
           labels.data_ptr(), is64, has_ignore, ignore, _ptr(u), code, float(beta), float(lam), int(k_reg), score.data_ptr(),
           rank.data_ptr(), n, c)
    return score, rank


@_device_guard()
def conformal_sets(logits: torch.Tensor, qhat: float, method: str = "aps", beta: float = 1.0, u: Optional[torch.Tensor] = None,
                   lam: float = 0.0, k_reg: int = 0, labels: Optional[torch.Tensor] = None, ignore_index: Optional[int] = None,
                   want_members: bool = True) -> ConformalSets:
    """The sets ``{c : s_c <= qhat}`` of logits [N, C] (``runia_conformal_sets``; C <= ``conformal_max_classes()``): the row is
    ordered inside the workgroup, the logits are read once.  With ``labels``, ``covered`` says whether the set holds the label."""
    require_gpu()
    logits, u, code = _conformal_rows(logits, u, method)
    n, c = logits.shape
    assert c <= conformal_max_classes(), f"C = {c} is above the limit of {conformal_max_classes()} classes"
    assert qhat == qhat, "qhat is NaN"
    labels, is64, has_ignore, ignore = _calib_labels(labels, n, ignore_index)
    dev = logits.device
    size = torch.empty((n,), dtype=torch.int32, device=dev)
    members = torch.empty((n, (c + 31) // 32), dtype=torch.int32, device=dev) if want_members else None
    covered = torch.empty((n,), dtype=torch.uint8, device=dev) if labels is not None else None
    launch("runia_conformal_sets", logits.data_ptr(), ELEM_DTYPE_CODES[logits.dtype], logits.stride(0) if n > 1 else c,
           _ptr(labels), is64, has_ignore, ignore, _ptr(u), code, float(beta), float(lam), int(k_reg), float(qhat),
           size.data_ptr(), _ptr(members), _ptr(covered), n, c)
    return ConformalSets(size, members, covered)


CONFORMAL_WIDE_MAX_CLASSES = 1 << 20  # runia_conformal_sets_wide: the fixed-point masses of a row fit 64 bits
CONFORMAL_WIDE_MAX_ROWS = 1 << 26


@_device_guard()
def conformal_sets_wide(table: torch.Tensor, dtype: torch.dtype, T: int, B: int, V: int, qhat: float, method: str = "aps",
                        beta: float = 1.0, u: Optional[torch.Tensor] = None, lam: float = 0.0, k_reg: int = 0,
                        labels: Optional[torch.Tensor] = None, ignore_index: Optional[int] = None,
                        want_members: bool = True) -> ConformalSets:
    """The sets ``{c : s_c <= qhat}`` of ``T`` steps of ``B`` rows of ``V`` logits behind the device step ``table`` [T, 2] int64
    of {row 0 pointer, row stride} (``runia_conformal_sets_wide``, any ``V`` up to 2^20: the row is not ordered, the cut is
    found by a radix descent).  Row ``b * T + t`` of the result is step ``t`` of row ``b``: ``size`` [B * T] reshapes to (B, T).
    ``u`` [B * T] float32 or None; ``labels`` (B, T) int32 / int64 token ids (any row stride) or None.  The caller keeps the
    tensors behind ``table`` alive."""
    require_gpu()
    assert table.is_cuda and table.dtype == torch.int64 and table.shape == (T, 2) and table.is_contiguous(), \
        f"table: a contiguous [{T}, 2] int64 device tensor"
    assert dtype in ELEM_DTYPE_CODES, f"dtype: float32, float16 or bfloat16, got {dtype}"
    assert method in CONFORMAL_METHODS, f"method: one of {tuple(CONFORMAL_METHODS)}, got {method!r}"
    assert T >= 1 and B >= 1 and 1 <= V <= CONFORMAL_WIDE_MAX_CLASSES and B * T <= CONFORMAL_WIDE_MAX_ROWS, \
        f"{T} steps of ({B}, {V}) logits exceed the kernel's size limits"
    assert qhat == qhat, "qhat is NaN"
    n, dev = B * T, table.device
    if u is not None:
        assert u.is_cuda and u.dtype == torch.float32 and u.shape == (n,), "u: a [B * T] float32 device tensor"
        u = u.contiguous()
    if labels is not None:
        assert labels.is_cuda and labels.dtype in (torch.int32, torch.int64) and labels.shape == (B, T)
        if T > 1 and labels.stride(1) != 1:
            labels = labels.contiguous()
    size = torch.empty((n,), dtype=torch.int32, device=dev)
    members = torch.empty((n, (V + 31) // 32), dtype=torch.int32, device=dev) if want_members else None
    covered = torch.empty((n,), dtype=torch.uint8, device=dev) if labels is not None else None
    launch("runia_conformal_sets_wide", table.data_ptr(), ELEM_DTYPE_CODES[dtype], T, B, V, _ptr(labels),
           int(labels is not None and labels.dtype == torch.int64), labels.stride(0) if labels is not None and B > 1 else T,
           int(ignore_index is not None), 0 if ignore_index is None else int(ignore_index), _ptr(u), CONFORMAL_METHODS[method],
           float(beta), float(lam), int(k_reg), float(qhat), size.data_ptr(), _ptr(members), _ptr(covered))
    return ConformalSets(size, members, covered)


@_device_guard()
def conformal_reduce(sets: ConformalSets, labels: torch.Tensor, c: int, ignore_index: Optional[int] = None) -> torch.Tensor:
    """``size`` / ``covered`` / labels -> the int64 device record of ``runia_conformal_reduce`` (``conformal_record`` splits a
    host copy)."""
    require_gpu()
    n = labels.shape[0]
    assert sets.covered is not None and sets.size.shape == (n,) and sets.covered.shape == (n,)
    labels, is64, has_ignore, ignore = _calib_labels(labels, n, ignore_index)
    out = torch.empty((query("runia_conformal_record_slots", c),), dtype=torch.int64, device=labels.device)
    launch("runia_conformal_reduce", sets.size.data_ptr(), sets.covered.data_ptr(), labels.data_ptr(), is64, has_ignore, ignore, n,
           c, out.data_ptr())
    return out


def conformal_record(record: np.ndarray, c: int) -> dict:
    """A host copy of ``conformal_reduce``'s record -> its named parts."""
    h = min(c + 1, 512)
    return {"n_used": int(record[0]), "n_covered": int(record[1]), "size_sum": int(record[2]), "hist": record[3:3 + h].copy(),
            "class_count": record[3 + h:3 + h + c].copy(), "class_covered": record[3 + h + c:3 + h + 2 * c].copy()}


@_device_guard()
def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    x = x.contiguous()
    y = torch.empty_like(x)
    launch("runia_l2_normalize_f32", x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1])
    return y


@_device_guard()
def knn_prepare_bank(bank: torch.Tensor) -> torch.Tensor:
    """Once per bank: squared row norms, their maximum and (banks the bf16 kernel can take) the bf16 pieces, as one
    device buffer for ``knn_kth(..., state=)``.  A deployed index scores many batches against the same bank; each call
    then skips the bank passes (50 000 x 2048: 0.4 ms)."""
    require_gpu()
    assert bank.is_cuda and bank.dtype == torch.float32 and bank.dim() == 2 and bank.is_contiguous()
    m, d = bank.shape
    nbytes = query("runia_knn_bank_state_bytes", m, d)
    state = torch.empty((max(nbytes, 16) + 15) // 16 * 4, dtype=torch.float32, device=bank.device)  # (16-byte granules)
    launch("runia_knn_prepare_bank_f32", bank.data_ptr(), state.data_ptr(), nbytes, m, d)
    return state


@_device_guard()
def knn_kth(q: torch.Tensor, bank: torch.Tensor, k: int, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [N, D], bank [M, D] (both L2-normalised f32) -> -(k-th smallest squared L2) [N] f32.
    ``state``: ``knn_prepare_bank(bank)`` of the same bank (same scores, without the per-call bank passes)."""
    lib = load_library()
    require_gpu()
    assert q.is_cuda and bank.is_cuda and q.dtype == torch.float32 and bank.dtype == torch.float32
    q = q.contiguous()
    bank = bank.contiguous()
    n, d = q.shape
    m = bank.shape[0]
    s = torch.empty((n,), dtype=torch.float32, device=q.device)
    f32_only = not _config.knn_bf16_candidates  # (hand the entry point the f32 kernel's workspace: it keeps that kernel)
    qc = min(n, 8192, max(256, (1 << 31) // (4 * m)))  # the f32 kernel's chunk of distances (+ |q|^2 ...)
    if state is not None and m > 0 and n > 0:
        ws_bytes = (qc * m + qc) * 4 if f32_only else int(lib.runia_knn_prepared_workspace_bytes(n, m, d, k))
        ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=q.device)
        launch("runia_knn_kth_prepared_f32", q.data_ptr(), bank.data_ptr(), state.data_ptr(), state.numel() * 4, s.data_ptr(),
               ws.data_ptr(), ws_bytes, n, m, d, int(k))
        return s
    ws_bytes = lib.runia_knn_workspace_bytes(n, m, d, k)
    if f32_only and lib.runia_knn_piece_products(n, m, d) > 0:
        # the f32 kernel's workspace (one chunk of distances, |q|^2, |b|^2, max |b|^2): the entry point then keeps that kernel
        ws_bytes = (qc * m + qc + m + 4) * 4
    ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=q.device)
    launch("runia_knn_kth_f32", q.data_ptr(), bank.data_ptr(), s.data_ptr(), ws.data_ptr(), ws_bytes, n, m, d, int(k))
    return s


@_device_guard()
def row_sqnorm(x: torch.Tensor) -> torch.Tensor:
    """x [N, D] f64 -> squared row norms [N] f64."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    x = x.contiguous()
    out = torch.empty((x.shape[0],), dtype=torch.float64, device=x.device)
    launch("runia_row_sqnorm_f64", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1])
    return out


@_device_guard()
def kde_pack_train(train: torch.Tensor):
    """Setup-time state of ``kde_score_packed``: (pack(train_c^T), squared row norms of train_c, M, D, mean) with
    train_c = train - mean(train).  Distances are translation invariant; centring keeps |x|^2 + |t|^2 - 2 x.t
    well conditioned when the embeddings sit far from the origin."""
    assert train.is_cuda and train.dtype == torch.float64 and train.dim() == 2
    mean = train.mean(dim=0)
    tc = (train - mean).contiguous()
    return pack_weights(tc.t().contiguous()), row_sqnorm(tc), int(train.shape[0]), int(train.shape[1]), mean


@_device_guard()
def kde_score_packed(state, x: torch.Tensor, bandwidth: float = 1.0) -> torch.Tensor:
    """Gaussian-KDE log-density [N] f64 of x [N, D] f64 against a packed training set (matrix-core path)."""
    require_gpu()
    packed, tn, m, d, mean = state
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == d
    x = (x - mean).contiguous()
    n = x.shape[0]
    out = torch.empty((n,), dtype=torch.float64, device=x.device)
    ws_bytes = query("runia_kde_workspace_bytes", n, m)  # query norms (+ the values of the column-split launch on few rows)
    ws = workspace(ws_bytes, x.device, 8)
    launch("runia_kde_score_packed_f64", packed.data_ptr(), tn.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes,
           m, n, d, float(bandwidth))
    return out


@_device_guard()
def kde_score(train: torch.Tensor, x: torch.Tensor, bandwidth: float = 1.0) -> torch.Tensor:
    """train [M, D] f64, x [N, D] f64 -> gaussian-KDE log-density [N] f64."""
    require_gpu()
    assert train.is_cuda and x.is_cuda and train.dtype == torch.float64 and x.dtype == torch.float64
    train = train.contiguous()
    x = x.contiguous()
    m, d = train.shape
    n = x.shape[0]
    s = torch.empty((n,), dtype=torch.float64, device=x.device)
    launch("runia_kde_score_f64", train.data_ptr(), x.data_ptr(), s.data_ptr(), m, n, d, float(bandwidth))
    return s


_TIMED_EVENT_POOL: dict = {}  # device index -> event pairs created (recorded once) on that device


def reserve_timed_events(n: int) -> None:
    """Create ``n`` event pairs for :func:`_timed_launch_events` now, on the current device (an event exists only once it has
    been recorded: two marker packets on the stream per pair), so that a bracketed launch inside a timed region costs no record of
    its own.  The pool is kept per device: an event belongs to the device it was first recorded on."""
    pool = _TIMED_EVENT_POOL.setdefault(torch.cuda.current_device(), [])
    for _ in range(int(n)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        pool.append((e0, e1))


def _timed_launch_events():
    """An event pair attached to the NEXT timed launch site (``runia_time_next_launch``): the events then hold the kernel's
    own start / end timestamps (what rocprofv3's kernel trace reports).  A pair recorded around the launch on the stream also
    counts the dispatch gap behind the previous kernel: K1 read 117.3 us that way against 109.5 us in the trace of the same run.
    Use :func:`_timed_call` around the entry point: it disarms the pair if the call returns before its launch site."""
    pool = _TIMED_EVENT_POOL.setdefault(torch.cuda.current_device(), [])
    if not pool:
        reserve_timed_events(1)
    e0, e1 = pool.pop()
    call("runia_time_next_launch", e0.cuda_event, e1.cuda_event)
    return e0, e1


def _timed_call(name: str, *args):
    """Arm an event pair, ``launch(name, *args)``, and ALWAYS disarm afterwards: an entry point that returns before its
    timed launch site (unsupported shape, short workspace) must not leave the pair to the thread's next, unrelated launch.
    Returns the pair; raises as ``launch`` does (the pair of a failed call never received timestamps and is dropped)."""
    e0, e1 = _timed_launch_events()
    try:
        launch(name, *args)
    finally:
        load_library().runia_time_next_launch(None, None)
    return e0, e1


def _launch_with_events(kernel_events: Optional[list], name: str, *args) -> None:
    """``launch(name, *args)``; given a list, the call runs under :func:`_timed_call` and its event pair is appended."""
    if kernel_events is not None:
        kernel_events.append(_timed_call(name, *args))
    else:
        launch(name, *args)


def mc_entropy_supported(h: int, w: int, n_mc: int, k: int) -> bool:
    return bool(query("runia_mc_entropy_supported", int(h), int(w), int(n_mc), int(k)))


@_device_guard()
def mc_mask_table(rand: Union[torch.Tensor, CounterDraws, None], n: int, h: int, w: int, n_mc: int, drop_prob: float,
                  block_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K0 alone: the keep-flag table of a batch of ``n`` <= 65 535 images (``runia_mc_mask_table_f32`` / its counter
    form) into ``out`` (uint8 workspace of ``runia_mc_entropy_workspace_bytes``) on the current stream.  Pass the result
    as ``table=`` to :func:`mc_entropy`: a caller that knows the next batch's draws builds its table on a side stream
    under the previous batch's kernels (``LaREMPipeline.prepare_draws``)."""
    lib = load_library()
    dev = require_gpu()
    assert 0 < n <= 65535
    ws_bytes = int(lib.runia_mc_entropy_workspace_bytes(n, h, w, n_mc))
    if out is None:
        out = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    assert out.is_cuda and out.dtype == torch.uint8 and out.numel() >= ws_bytes
    if isinstance(rand, CounterDraws):
        launch("runia_mc_mask_table_counter_f32", int(rand.seed) & (2**64 - 1), int(rand.first_image), out.data_ptr(), ws_bytes,
               n, h, w, n_mc, float(drop_prob), int(block_size), int(bool(rand.redraw_dead_layers)))
        return out
    rand, stride = _draws(rand, n, n_mc, h, w, copy=False)
    launch("runia_mc_mask_table_f32", _ptr(rand), stride, out.data_ptr(), ws_bytes, n, h, w, n_mc,
           float(drop_prob) if rand is not None else 0.0, int(block_size))
    return out


_FLAG_LUTS: dict = {}  # (device index, H, W, block_size) -> device copy of the geometry table
_FLAG_LUTS_LOCK = threading.Lock()


def mc_flag_lut_host(h: int, w: int, block_size: int) -> np.ndarray:
    """The geometry table of ``runia_mc_flag_lut_fill`` as a [records, 20] uint32 array (no GPU needed): row ``key`` < 65 536 is
    the record of seed word ``key``, the rows behind them are zero padding (see ``runia_hip.h``)."""
    nbytes = query("runia_mc_flag_lut_bytes", int(h), int(w), int(block_size))
    if nbytes == 0:
        raise RuniaHipError(f"no keep-flag geometry table for {h}x{w} maps, block_size {block_size}")
    host = np.empty(nbytes // 4, dtype=np.uint32)
    call("runia_mc_flag_lut_fill", host.ctypes.data, nbytes, int(h), int(w), int(block_size))
    return host.reshape(-1, 20)


def _flag_lut(device: torch.device, h: int, w: int, block_size: int) -> torch.Tensor:
    """One device copy of the geometry table per (device, H, W, block_size): uploaded once, and the device synchronised once
    after the upload, because later launches that read it may come from any of the pipeline's streams."""
    key = (device.index, int(h), int(w), int(block_size))
    lut = _FLAG_LUTS.get(key)
    if lut is None:
        with _FLAG_LUTS_LOCK:
            lut = _FLAG_LUTS.get(key)
            if lut is None:
                lut = torch.from_numpy(mc_flag_lut_host(h, w, block_size).view(np.int32)).to(device)
                torch.cuda.synchronize(device)
                _FLAG_LUTS[key] = lut
    return lut


def mc_entropy_lut_supported(h: int, w: int, n_mc: int, k: int, block_size: int) -> bool:
    return bool(query("runia_mc_entropy_lut_supported", int(h), int(w), int(n_mc), int(k), int(block_size)))


@_device_guard()
def mc_entropy(x: torch.Tensor, rand: Union[torch.Tensor, CounterDraws, None], n_mc: int, drop_prob: float, block_size: int, k: int,
               min_dist: float = 1e-5, want_samples: bool = False, out: Optional[torch.Tensor] = None,
               kernel_events: Optional[list] = None, zero_fill: Optional[torch.Tensor] = None,
               table: Optional[torch.Tensor] = None):
    """Fused sampler + entropy: x [N,C,H,W] f32 (+ draws) -> h [N, C] f64 (and optionally the MC samples).
    ``kernel_events``: if a list, (start, end) HIP event pairs attached to the dispatch of the sampler + entropy launch
    (the kernel's own start / end timestamps; the keep-flag table launch before it is left out) are appended - bench.py
    times the dominant kernel with it.
    ``zero_fill``: optional [N] f64 tensor cleared by the launch (the accumulator of ``proj_sq_accumulate``).
    ``table``: the batch's keep-flag table built earlier by :func:`mc_mask_table` (``rand`` is then ignored).
    The product case - 4x4 maps, 16 drop layers, k = 5, ``rand`` a tensor, ``drop_prob > 0``, no samples, no ``table`` - is ONE
    launch that reads the draws itself (``runia_mc_entropy_lut_f32``; ``config.k1_flag_table``), with or without
    ``kernel_events``; everything else is the keep-flag table launch + the launch from that table.  Same bits either way."""
    lib = load_library()
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n, c, hh, ww = x.shape
    h = torch.empty((n, c), dtype=torch.float64, device=x.device) if out is None else out
    assert h.is_cuda and h.dtype == torch.float64 and h.shape == (n, c) and h.is_contiguous()
    z = torch.empty((n * n_mc, c), dtype=torch.float32, device=x.device) if want_samples else None
    if zero_fill is not None:
        assert zero_fill.is_cuda and zero_fill.dtype == torch.float64 and zero_fill.shape == (n,) and zero_fill.is_contiguous()
    if table is not None:
        ws_bytes = int(lib.runia_mc_entropy_workspace_bytes(n, hh, ww, n_mc))
        assert table.is_cuda and table.numel() >= ws_bytes and n <= 65535
        _launch_with_events(kernel_events, "runia_mc_entropy_from_table_f32", x.data_ptr(), table.data_ptr(), ws_bytes,
                            h.data_ptr(), _ptr(z), _ptr(zero_fill), n, c, hh, ww, n_mc, int(k), float(min_dist))
        return (h, z) if want_samples else h
    counter = rand if isinstance(rand, CounterDraws) else None
    rand, stride = _draws(None if counter is not None else rand, n, n_mc, hh, ww)
    if (_config.k1_flag_table and rand is not None and not want_samples and drop_prob > 0 and x.data_ptr() % 16 == 0
            and mc_entropy_lut_supported(hh, ww, n_mc, k, block_size)):
        # the product case: one launch from the draws and the geometry table (no keep-flag launch, no per-image table)
        lut = _flag_lut(x.device, hh, ww, block_size)
        lut_bytes = lut.numel() * 4
        for done, m in _image_slices(n):
            _launch_with_events(kernel_events, "runia_mc_entropy_lut_f32", x.data_ptr() + done * c * hh * ww * 4,
                                rand.data_ptr() + done * stride * 4, stride, lut.data_ptr(), lut_bytes, h.data_ptr() + done * c * 8,
                                None if zero_fill is None else zero_fill.data_ptr() + done * 8, m, c, hh, ww, n_mc,
                                float(drop_prob), int(block_size), int(k), float(min_dist))
        return h
    ws_bytes = int(lib.runia_mc_entropy_workspace_bytes(min(65535, n), hh, ww, n_mc))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)  # stream-ordered: reused per slice
    if counter is not None:
        seed, redraw = int(counter.seed) & (2**64 - 1), int(bool(counter.redraw_dead_layers))
    for done, m in _image_slices(n):
        xp, hp = x.data_ptr() + done * c * hh * ww * 4, h.data_ptr() + done * c * 8
        rp = None if rand is None else rand.data_ptr() + done * stride * 4
        zp = None if z is None else z.data_ptr() + done * n_mc * c * 4
        zf = None if zero_fill is None else zero_fill.data_ptr() + done * 8
        if kernel_events is not None:  # the keep-flag table on its own, then the timed sampler + entropy launch
            if counter is not None:
                launch("runia_mc_mask_table_counter_f32", seed, int(counter.first_image) + done, ws.data_ptr(), ws_bytes, m, hh,
                       ww, n_mc, float(drop_prob), int(block_size), redraw)
            else:
                launch("runia_mc_mask_table_f32", rp, stride, ws.data_ptr(), ws_bytes, m, hh, ww, n_mc, float(drop_prob),
                       int(block_size))
            _launch_with_events(kernel_events, "runia_mc_entropy_from_table_f32", xp, ws.data_ptr(), ws_bytes, hp, zp, zf, m, c,
                                hh, ww, n_mc, int(k), float(min_dist))
        elif counter is not None:
            launch("runia_mc_entropy_counter_f32", xp, seed, int(counter.first_image) + done, hp, zp, zf, ws.data_ptr(), ws_bytes,
                   m, c, hh, ww, n_mc, float(drop_prob), int(block_size), int(k), float(min_dist), redraw)
        else:
            launch("runia_mc_entropy_f32", xp, rp, stride, hp, zp, zf, ws.data_ptr(), ws_bytes, m, c, hh, ww, n_mc,
                   float(drop_prob), int(block_size), int(k), float(min_dist))
    return (h, z) if want_samples else h


def _proj_sq_entry(kind: str, trap: bool, balanced: bool) -> str:
    if balanced and not trap:
        raise ValueError("balanced=True describes an upper-trapezoidal matrix: pass trap=True with it")
    return f"runia_proj_sq_{kind}_{'btrap_' if balanced else 'trap_' if trap else ''}f64"


@_device_guard()
def proj_sq_accumulate(h: torch.Tensor, packed_m: torch.Tensor, c: torch.Tensor, r: int, out: torch.Tensor,
                       trap: bool = False, balanced: bool = False) -> torch.Tensor:
    """``out`` [N] f64 += -|| M h + c ||^2 where ``out`` was zeroed earlier on the stream (``mc_entropy(zero_fill=out)``):
    the score of ``proj_sq_score`` bit for bit, without its workspace and combine launch.  ``trap``: M is upper-trapezoidal
    (``qr_trapezoid``); the launch skips its zero blocks (``runia_proj_sq_accumulate_trap_f64``).  ``balanced`` (with
    ``trap``): its row blocks stand in the balanced order (``trap_balance_rows``; ``runia_proj_sq_accumulate_btrap_f64``)."""
    require_gpu()
    assert h.is_cuda and h.dtype == torch.float64 and h.dim() == 2
    h = h.contiguous()
    nrow, d = h.shape
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (nrow,) and out.is_contiguous()
    launch(_proj_sq_entry("accumulate", trap, balanced), h.data_ptr(), packed_m.data_ptr(),
           c.data_ptr(), out.data_ptr(), nrow, d, int(r))
    return out


@_device_guard()
def pca_md_score(h: torch.Tensor, packed_ct: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                 scale: Optional[torch.Tensor], md_mean: torch.Tensor, packed_p: torch.Tensor, n: int,
                 want_projection: bool = False, out: Optional[torch.Tensor] = None):
    """Fused PCA transform + LaREM score: h [N, D] f64 -> score [N] f64 (projected rows stay on chip)."""
    require_gpu()
    assert h.is_cuda and h.dtype == torch.float64 and h.dim() == 2
    h = h.contiguous()
    nrow, d = h.shape
    if out is None:
        s = torch.empty((nrow,), dtype=torch.float64, device=h.device)
    else:
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (nrow,) and out.is_contiguous()
        s = out
    y = torch.empty((nrow, n), dtype=torch.float64, device=h.device) if want_projection else None
    launch("runia_pca_md_score_f64", h.data_ptr(), _ptr(packed_ct), _ptr(bias), _ptr(scale), md_mean.data_ptr(),
           packed_p.data_ptr(), s.data_ptr(), _ptr(y), nrow, d, n)
    return (s, y) if want_projection else s


@_device_guard()
def covariance(x: torch.Tensor):
    """x [N, D] f64/f32 (device) -> (mean [D] f64, cov [D, D] f64) = np.cov(x.T, bias=1) with its column means."""
    require_gpu()
    assert x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64)
    x = x.contiguous()
    n, d = x.shape
    mean = torch.empty((d,), dtype=torch.float64, device=x.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=x.device)
    ws_bytes = query("runia_covariance_workspace_bytes", n, d)
    ws = workspace(ws_bytes, x.device, 8)
    launch("runia_covariance_f32in" if x.dtype == torch.float32 else "runia_covariance_f64", x.data_ptr(), mean.data_ptr(),
           cov.data_ptr(), ws.data_ptr(), ws_bytes, n, d)
    return mean, cov


@_device_guard()
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], clip_max: float = float("inf")) -> torch.Tensor:
    """logits [N, C] = min(x, clip_max) @ w.T + bias  (x [N, D], w [C, D], all f32 on the device)."""
    require_gpu()
    assert x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.shape[1] == w.shape[1]
    x, w = x.contiguous(), w.contiguous()
    n, d = x.shape
    c = w.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    launch("runia_linear_f32", x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), n, d, c, float(clip_max))
    return out


@_device_guard()
def ash_s(x: torch.Tensor, percentile: int) -> torch.Tensor:
    """ASH-S of 2-D activations (``ash_s_linear_layer``): rows of up to 4 096 features in registers (wave per row), longer
    rows through the radix-select kernel (workgroup per row)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.shape[1] <= 4096:
        launch("runia_ash_s_f32", x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], int(percentile))
    else:
        launch("runia_ash_s_rows_f32", x.data_ptr(), y.data_ptr(), None, x.shape[0], x.shape[1], int(percentile), 1)
    return y


@_device_guard()
def ash_s_conv(x: torch.Tensor, percentile: int, prune_in_place: bool = True) -> torch.Tensor:
    """ASH-S of (B, C, H, W) maps (``ash_s_conv_layer``): per sample the k largest of its C*H*W activations are kept and
    the sample is multiplied by exp(sum / kept sum).  ``prune_in_place``: ``x`` itself is left pruned, as the
    reference's ``view`` + ``scatter_`` leaves its argument (x must then be contiguous)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    assert x.is_contiguous() or not prune_in_place
    xc = x.contiguous()
    b = xc.shape[0]
    d = xc.numel() // max(b, 1)
    y = torch.empty_like(xc)
    launch("runia_ash_s_rows_f32", xc.data_ptr(), y.data_ptr(), xc.data_ptr() if prune_in_place else None, b, d, int(percentile),
           0)
    return y


@_device_guard()
def gen_entropy(probs: torch.Tensor, gamma: float, m: int) -> torch.Tensor:
    """``generalized_entropy(probs, gamma, M)`` on rows that already are probabilities -> [N] f32."""
    require_gpu()
    assert probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2
    probs = probs.contiguous()
    s = torch.empty((probs.shape[0],), dtype=torch.float32, device=probs.device)
    launch("runia_gen_entropy_f32", probs.data_ptr(), s.data_ptr(), probs.shape[0], probs.shape[1], int(m), float(gamma))
    return s


@_device_guard()
def mcd_uncertainty(logits: torch.Tensor, n_mc: int, want_probs: bool = False):
    """logits [N * n_mc, C] f32 (an image's MC rows consecutive) -> (pred_h [N], mi [N], softmax rows or None): the
    predictive entropy of the mean distribution and the mutual information, one launch."""
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[0] % n_mc == 0
    logits = logits.contiguous()
    n, c = logits.shape[0] // n_mc, logits.shape[1]
    ph = torch.empty((n,), dtype=torch.float32, device=logits.device)
    mi = torch.empty((n,), dtype=torch.float32, device=logits.device)
    probs = torch.empty_like(logits) if want_probs else None
    launch("runia_mcd_uncertainty_f32", logits.data_ptr(), _ptr(probs), ph.data_ptr(), mi.data_ptr(), n, int(n_mc), c)
    return ph, mi, probs


PIXEL_MAP_SCORES = ("pred_h", "mi", "msp", "energy", "max_logit")


@_device_guard()
def pixel_uncertainty_maps(passes, n_mc: int, scores=("pred_h", "mi"), want_label: bool = False,
                           want_mean_probs: bool = False):
    """Per-pixel maps of a segmentation head, one launch (``runia_pixel_uncertainty_maps``).  ``passes``: ONE device tensor
    (G * n_mc, C, H, W) whose rows g * n_mc + s are the samples of image g, or a list / tuple of ``n_mc`` device tensors
    (G, C, H, W) of one shape, dtype (f32 / f16 / bf16) and stride tuple; any strides, read in place.  Returns a dict with
    the requested ``scores`` (f32 (G, H, W)) and, when asked for, ``"label"`` (int32 (G, H, W)) and ``"mean_probs"`` (f32
    (G, C, H, W)).  ``0 * log 0`` is NaN as in ``mcd_uncertainty``."""
    single = isinstance(passes, torch.Tensor)
    first = passes if single else passes[0]
    n_mc = int(n_mc)
    assert all(s in PIXEL_MAP_SCORES for s in scores), f"scores must be among {PIXEL_MAP_SCORES}"
    assert first.dim() == 4 and first.dtype in ELEM_DTYPE_CODES and first.is_cuda
    if single:
        assert first.shape[0] % n_mc == 0
        g = first.shape[0] // n_mc
    else:
        assert len(passes) == n_mc and all(
            t.is_cuda and t.device == first.device and t.shape == first.shape and t.dtype == first.dtype
            and t.stride() == first.stride() for t in passes)
        g = first.shape[0]
    require_gpu()
    _, c, h, w = (int(v) for v in first.shape)
    dev = first.device
    out = {s: torch.empty((g, h, w), dtype=torch.float32, device=dev) for s in scores}
    if want_label:
        out["label"] = torch.empty((g, h, w), dtype=torch.int32, device=dev)
    if want_mean_probs:
        out["mean_probs"] = torch.empty((g, c, h, w), dtype=torch.float32, device=dev)
    if g == 0 or h * w == 0:
        return out
    assert out, "at least one map must be requested"
    table = torch.tensor([first.data_ptr()] if single else [t.data_ptr() for t in passes], dtype=torch.int64).to(dev)
    need = query("runia_pixel_maps_workspace_bytes", g, c, h, w, n_mc, int("max_logit" in out))
    ws = workspace(need, dev, 0) if need else None
    sn, sc, sh, sw = (int(v) for v in first.stride())
    launch("runia_pixel_uncertainty_maps", table.data_ptr(), int(single), ELEM_DTYPE_CODES[first.dtype], g, n_mc, c, h, w, sn, sc,
           sh, sw, _ptr(out.get("pred_h")), _ptr(out.get("mi")), _ptr(out.get("msp")), _ptr(out.get("energy")),
           _ptr(out.get("max_logit")), _ptr(out.get("label")), _ptr(out.get("mean_probs")), _ptr(ws), need)
    return out


@_device_guard()
def pixel_map_reduce(score_map: torch.Tensor, valid: Optional[torch.Tensor] = None):
    """Per-image (mean, max, count) of a (G, H, W) f32 device map under an optional (G, H, W) bool / uint8 validity mask ->
    (f32 (G,), f32 (G,), int64 (G,)); deterministic.  An image without a valid pixel gives (NaN, -inf, 0)."""
    assert score_map.is_cuda and score_map.dtype == torch.float32 and score_map.dim() == 3
    require_gpu()
    m = score_map.contiguous()
    g, hw = int(m.shape[0]), int(m.shape[1] * m.shape[2])
    v = None
    if valid is not None:
        assert tuple(valid.shape) == tuple(m.shape) and valid.dtype in (torch.bool, torch.uint8)
        v = valid.to(m.device).contiguous().view(torch.uint8)
    mean = torch.empty((g,), dtype=torch.float32, device=m.device)
    mx = torch.empty((g,), dtype=torch.float32, device=m.device)
    cnt = torch.empty((g,), dtype=torch.int64, device=m.device)
    launch("runia_pixel_map_reduce_f32", m.data_ptr(), _ptr(v), g, hw, mean.data_ptr(), mx.data_ptr(), cnt.data_ptr())
    return mean, mx, cnt


PIXFEAT_OUTPUTS = ("distance", "nearest", "class_distances")
PIXFEAT_MAX_CHANNELS, PIXFEAT_MAX_CLASSES = 1024, 256  # the limits of runia_pixfeat_score
# label dtype of the maps -> the `label_dtype` code of runia_pixfeat_label_hist / runia_pixfeat_gather_rows
PIXFEAT_LABEL_CODES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}


@_device_guard()
def pixfeat_score(features: torch.Tensor, m0: torch.Tensor, w: torch.Tensor, mz: torch.Tensor, outputs=("distance",)):
    """Per-pixel Mahalanobis maps, one launch (``runia_pixfeat_score``).  ``features`` (G, C, h, w) f32 / f16 / bf16 on the
    device, any strides, read in place; ``m0`` [C], ``w`` [C, C] lower triangular, ``mz`` [K, C] f32 on the device (a row
    of ``+inf`` excludes its class).  Returns a dict with the requested ``outputs``: ``"distance"`` f32 (G, h, w),
    ``"nearest"`` int32 (G, h, w), ``"class_distances"`` f32 (G, K, h, w)."""
    assert all(o in PIXFEAT_OUTPUTS for o in outputs) and len(outputs) > 0, f"outputs must be among {PIXFEAT_OUTPUTS}"
    assert features.is_cuda and features.dim() == 4 and features.dtype in ELEM_DTYPE_CODES
    g, c, h, wd = (int(v) for v in features.shape)
    k = int(mz.shape[0])
    for t, shape in ((m0, (c,)), (w, (c, c)), (mz, (k, c))):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
    require_gpu()
    dev = features.device
    out = {}
    if "distance" in outputs:
        out["distance"] = torch.empty((g, h, wd), dtype=torch.float32, device=dev)
    if "nearest" in outputs:
        out["nearest"] = torch.empty((g, h, wd), dtype=torch.int32, device=dev)
    if "class_distances" in outputs:
        out["class_distances"] = torch.empty((g, k, h, wd), dtype=torch.float32, device=dev)
    need = query("runia_pixfeat_workspace_bytes", c, k)
    ws = workspace(need, dev, 0) if need else None
    sn, sc, sh, sw = (int(v) for v in features.stride())
    launch("runia_pixfeat_score", features.data_ptr(), ELEM_DTYPE_CODES[features.dtype], g, c, h, wd, sn, sc, sh, sw,
           m0.data_ptr(), w.data_ptr(), mz.data_ptr(), k, _ptr(out.get("distance")), _ptr(out.get("nearest")),
           _ptr(out.get("class_distances")), _ptr(ws), need)
    return out


def _pixfeat_labels(labels: torch.Tensor) -> torch.Tensor:
    assert labels.is_cuda and labels.dim() == 3 and labels.dtype in PIXFEAT_LABEL_CODES, \
        f"labels: a (G, h, w) device tensor of int64, int32 or uint8, got {tuple(labels.shape)} {labels.dtype}"
    return labels.contiguous()


@_device_guard()
def pixfeat_label_hist(labels: torch.Tensor, n_classes: int, ignore_index: int = 255):
    """labels (G, h, w) int64 / int32 / uint8 on the device -> (counts int64 [n_classes], dropped int64 [1]) on the device:
    the pixels per class, and those ignored or outside ``[0, n_classes)``."""
    labels = _pixfeat_labels(labels)
    require_gpu()
    counts = torch.empty((int(n_classes),), dtype=torch.int64, device=labels.device)
    dropped = torch.empty((1,), dtype=torch.int64, device=labels.device)
    launch("runia_pixfeat_label_hist", labels.data_ptr(), PIXFEAT_LABEL_CODES[labels.dtype], labels.numel(), int(n_classes),
           int(ignore_index), counts.data_ptr(), dropped.data_ptr())
    return counts, dropped


@_device_guard()
def pixfeat_gather_rows(features: torch.Tensor, labels: torch.Tensor, keep_prob: torch.Tensor, ignore_index: int = 255,
                        seed: int = 0, image_offset: int = 0):
    """The labelled pixels of ``features`` (G, C, h, w) kept by the counter draw (``runia_pixfeat_gather_rows``) ->
    ``(rows f32 (n, C), row_labels int32 (n,))`` on the device, in pixel order.  ``keep_prob`` f32 [K] on the device.  The
    count is read back once (a host synchronisation) to size the table."""
    assert features.is_cuda and features.dim() == 4 and features.dtype in ELEM_DTYPE_CODES
    labels = _pixfeat_labels(labels)
    g, c, h, wd = (int(v) for v in features.shape)
    assert tuple(labels.shape) == (g, h, wd), f"labels {tuple(labels.shape)} do not match the features {(g, h, wd)}"
    assert keep_prob.is_cuda and keep_prob.dtype == torch.float32 and keep_prob.dim() == 1 and keep_prob.is_contiguous()
    require_gpu()
    dev = features.device
    k = int(keep_prob.shape[0])
    n_out = torch.zeros((1,), dtype=torch.int64, device=dev)
    need = query("runia_pixfeat_gather_workspace_bytes", g * h * wd)
    ws = workspace(need, dev, 8)
    sn, sc, sh, sw = (int(v) for v in features.stride())
    head = (features.data_ptr(), ELEM_DTYPE_CODES[features.dtype], g, c, h, wd, sn, sc, sh, sw, labels.data_ptr(),
            PIXFEAT_LABEL_CODES[labels.dtype], k, int(ignore_index), keep_prob.data_ptr(), int(seed) & ((1 << 64) - 1),
            int(image_offset))
    launch("runia_pixfeat_gather_rows", *head, None, None, 0, n_out.data_ptr(), ws.data_ptr(), need)
    n = int(n_out.item())
    rows = torch.empty((n, c), dtype=torch.float32, device=dev)
    row_labels = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        launch("runia_pixfeat_gather_rows", *head, rows.data_ptr(), row_labels.data_ptr(), n, n_out.data_ptr(), ws.data_ptr(),
               need)
    return rows, row_labels


PIXKNN_OUTPUTS = ("kth_distance", "mean_distance", "distances", "indices")
PIXKNN_MAX_CHANNELS, PIXKNN_MAX_K, PIXKNN_MAX_BANK = 1024, 16, 1 << 22  # the limits of runia_pixknn_score
KCENTER_MAX_COLUMNS = 1024                                               # and of runia_kcenter_greedy_f32


@_device_guard()
def pixknn_score(features: torch.Tensor, center: torch.Tensor, bank: torch.Tensor, bank_sq: torch.Tensor, k: int,
                 outputs=("kth_distance",)):
    """Per-pixel kNN maps, one launch (``runia_pixknn_score``).  ``features`` (G, C, h, w) f32 / f16 / bf16 on the device, any
    strides, read in place; ``center`` [C], ``bank`` [M, C] (already centred) and ``bank_sq`` [M] (its squared row norms) f32
    on the device.  Returns a dict with the requested ``outputs``: ``"distances"`` f32 (G, k, h, w) ascending, ``"indices"``
    int32 (G, k, h, w), ``"kth_distance"`` and ``"mean_distance"`` f32 (G, h, w).  Squared Euclidean distances."""
    assert all(o in PIXKNN_OUTPUTS for o in outputs) and len(outputs) > 0, f"outputs must be among {PIXKNN_OUTPUTS}"
    assert features.is_cuda and features.dim() == 4 and features.dtype in ELEM_DTYPE_CODES
    g, c, h, wd = (int(v) for v in features.shape)
    m, k = int(bank.shape[0]), int(k)
    for t, shape in ((center, (c,)), (bank, (m, c)), (bank_sq, (m,))):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
    require_gpu()
    dev = features.device
    shapes = {"kth_distance": ((g, h, wd), torch.float32), "mean_distance": ((g, h, wd), torch.float32),
              "distances": ((g, k, h, wd), torch.float32), "indices": ((g, k, h, wd), torch.int32)}
    out = {o: torch.empty(shapes[o][0], dtype=shapes[o][1], device=dev) for o in PIXKNN_OUTPUTS if o in outputs}
    need = query("runia_pixknn_workspace_bytes", c, m, k)
    ws = workspace(need, dev, 0) if need else None
    sn, sc, sh, sw = (int(v) for v in features.stride())
    launch("runia_pixknn_score", features.data_ptr(), ELEM_DTYPE_CODES[features.dtype], g, c, h, wd, sn, sc, sh, sw,
           center.data_ptr(), bank.data_ptr(), bank_sq.data_ptr(), m, k, _ptr(out.get("distances")), _ptr(out.get("indices")),
           _ptr(out.get("kth_distance")), _ptr(out.get("mean_distance")), _ptr(ws), need)
    return {o: out[o] for o in outputs}


@_device_guard()
def kcenter_greedy(rows: torch.Tensor, n_pick: int, first: int = 0):
    """Greedy k-center selection (``runia_kcenter_greedy_f32``): ``rows`` f32 (N, D) contiguous on the device -> ``(picked
    int32 [n_pick], radius f32 [n_pick], n_picked int64 [1])`` on the device, nothing read back.  One launch per pick."""
    assert rows.is_cuda and rows.dim() == 2 and rows.dtype == torch.float32 and rows.is_contiguous()
    n, d = (int(v) for v in rows.shape)
    n_pick, first = int(n_pick), int(first)
    require_gpu()
    dev = rows.device
    picked = torch.empty((n_pick,), dtype=torch.int32, device=dev)
    radius = torch.empty((n_pick,), dtype=torch.float32, device=dev)
    n_picked = torch.zeros((1,), dtype=torch.int64, device=dev)
    need = query("runia_kcenter_workspace_bytes", n, d)
    ws = workspace(need, dev)
    launch("runia_kcenter_greedy_f32", rows.data_ptr(), n, d, first, n_pick, picked.data_ptr(), radius.data_ptr(),
           n_picked.data_ptr(), ws.data_ptr(), need)
    return picked, radius, n_picked


# (RUNIA_CC_TILE_H, RUNIA_CC_TILE_W) of include/runia_hip.h: the tile one workgroup of the labelling kernel owns
CC_TILE = (_HEADER_MACROS["RUNIA_CC_TILE_H"], _HEADER_MACROS["RUNIA_CC_TILE_W"])
CC_MAX_PIXELS = (1 << 31) - 1  # N * H * W of one labelling call (parents are int32)


def _cc_bytes(t: Optional[torch.Tensor], shape, name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    assert t.is_cuda and tuple(t.shape) == tuple(shape) and t.dtype in (torch.bool, torch.uint8), name
    return t.contiguous().view(torch.uint8)


@_device_guard()
def cc_label(mask: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
             thresholds: Optional[torch.Tensor] = None, less: bool = False, valid: Optional[torch.Tensor] = None,
             connectivity: int = 8):
    """Connected components of N binary images (``runia_cc_label``) -> (labels int32 (N, H, W), counts int32 (N,)): 0 is
    background, 1 .. counts[n] in raster order of each component's first pixel.  Either ``mask`` (N, H, W) bool / uint8, or
    ``score`` (G, H, W) f32 with ``thresholds`` (T,) f32: N = T * G, image t * G + g is ``score[g] > thresholds[t]``
    (``less``: <).  ``valid`` has the shape of the mask / of the score map.  Waits for the stream (the step caps' error word)."""
    assert (mask is None) != (score is None) and connectivity in (4, 8)
    src = mask if score is None else score
    assert src.is_cuda and src.dim() == 3
    require_gpu()
    g, h, w = (int(v) for v in src.shape)
    dev = src.device
    if score is None:
        m, sc, thr, t = _cc_bytes(mask, src.shape, "mask"), None, None, 1
    else:
        assert score.dtype == torch.float32 and thresholds.is_cuda and thresholds.dtype == torch.float32 and thresholds.dim() == 1
        m, sc, thr, t = None, score.contiguous(), thresholds.contiguous(), int(thresholds.shape[0])
    v = _cc_bytes(valid, src.shape, "valid")
    n = g * t
    assert n * h * w <= CC_MAX_PIXELS, "N * H * W of one labelling call must stay below 2^31"
    labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    counts = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n == 0 or h * w == 0:
        return labels, counts
    need = query("runia_cc_label_workspace_bytes", n, h, w)
    ws = workspace(need, dev)
    launch("runia_cc_label", _ptr(m), _ptr(sc), _ptr(thr), t, int(bool(less)), _ptr(v), g, h, w, int(connectivity),
           labels.data_ptr(), counts.data_ptr(), ws.data_ptr(), need)
    return labels, counts


def _cc_offsets(counts: torch.Tensor) -> torch.Tensor:
    return (torch.cumsum(counts, 0, dtype=torch.int64) - counts).to(torch.int32)


@_device_guard()
def cc_overlap(gt_labels: Optional[torch.Tensor], gt_counts: Optional[torch.Tensor], pred_labels: Optional[torch.Tensor],
               pred_counts: Optional[torch.Tensor], want_gt_size: bool = True):
    """Integer overlap tables of label images (``runia_cc_overlap``): ``gt_labels`` (G, H, W) and ``pred_labels`` (T * G, H, W)
    (image t * G + g) with their per-image ``counts``; either may be None.  Returns a dict of device tensors: ``gt_size``
    (Kg,), ``gt_inter`` (T, Kg), ``pred_size`` / ``pred_inter`` (Kp,) int32, ``pairs`` int64 (P,) - the distinct
    ``(t * Kg + k) << 32 | k_hat`` keys, ascending - and the offsets.  Components are rows in image order."""
    first = gt_labels if gt_labels is not None else pred_labels
    assert first is not None and first.is_cuda and first.dim() == 3 and first.dtype == torch.int32
    require_gpu()
    dev = first.device
    h, w = int(first.shape[1]), int(first.shape[2])
    out = {}
    g = int(gt_labels.shape[0]) if gt_labels is not None else int(pred_labels.shape[0])
    t = 0
    kg = kp = 0
    goff = poff = None
    if gt_labels is not None:
        assert gt_labels.is_contiguous() and gt_counts.dtype == torch.int32 and gt_counts.shape == (g,)
        goff = _cc_offsets(gt_counts)
    if pred_labels is not None:
        assert pred_labels.is_contiguous() and pred_labels.dtype == torch.int32 and tuple(pred_labels.shape[1:]) == (h, w)
        t = int(pred_labels.shape[0]) // g if g else 0
        assert pred_labels.shape[0] == g * t and pred_counts.dtype == torch.int32 and pred_counts.shape == (g * t,)
        poff = _cc_offsets(pred_counts)
    totals = [int(c.sum().item()) if c is not None else 0 for c in (gt_counts, pred_counts)]  # (one wait for both tables' sizes)
    kg, kp = totals

    def table(rows, wanted=True):  # (never an empty allocation: its null address would read as "not wanted")
        return torch.zeros((max(rows, 1),), dtype=torch.int32, device=dev) if wanted else None

    gt_size_b = table(kg, gt_labels is not None and want_gt_size)
    gt_inter_b = table(t * kg, gt_labels is not None)
    pred_size_b, pred_inter_b = table(kp, pred_labels is not None), table(kp, pred_labels is not None)
    n_keys = torch.zeros((1,), dtype=torch.int64, device=dev)
    pairs = torch.empty((0,), dtype=torch.int64, device=dev)
    if g > 0 and h * w > 0 and (gt_labels is None or pred_labels is None or t > 0):
        args = (_ptr(gt_labels), _ptr(goff), _ptr(pred_labels), _ptr(poff), g, t, h, w, kg)
        launch("runia_cc_overlap", *args, _ptr(gt_size_b), _ptr(gt_inter_b), _ptr(pred_size_b), _ptr(pred_inter_b), None, 0,
               n_keys.data_ptr(), 1)
        cand = int(n_keys.item()) if (gt_labels is not None and pred_labels is not None) else 0
        if cand:
            keys = torch.empty((cand,), dtype=torch.int64, device=dev)
            n_keys.zero_()
            launch("runia_cc_overlap", *args, None, None, None, None, keys.data_ptr(), cand, n_keys.data_ptr(), 0)
            pairs = torch.unique(keys)  # sorted: the result does not depend on the order the candidates arrived in
    gt_size = None if gt_size_b is None else gt_size_b[:kg]
    gt_inter = None if gt_inter_b is None else gt_inter_b[:t * kg].view(t, kg)
    pred_size = None if pred_size_b is None else pred_size_b[:kp]
    pred_inter = None if pred_inter_b is None else pred_inter_b[:kp]
    out.update(gt_size=gt_size, gt_inter=gt_inter, pred_size=pred_size, pred_inter=pred_inter, pairs=pairs, gt_offsets=goff,
               pred_offsets=poff, n_gt=kg, n_pred=kp)
    return out


@_device_guard()
def cc_relabel(labels: torch.Tensor, offsets: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """``labels[n, p] = table[offsets[n] + labels[n, p] - 1]`` where the label is positive, in place (``runia_cc_relabel``)."""
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.dim() == 3 and labels.is_contiguous()
    assert offsets.dtype == torch.int32 and table.dtype == torch.int32 and offsets.shape == (labels.shape[0],)
    require_gpu()
    n, h, w = (int(v) for v in labels.shape)
    if n and h * w and table.numel():
        launch("runia_cc_relabel", labels.data_ptr(), offsets.contiguous().data_ptr(), table.contiguous().data_ptr(), n, h, w)
    return labels


@_device_guard()
def gen_score(logits: torch.Tensor, gamma: float, m: int) -> torch.Tensor:
    require_gpu()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    logits = logits.contiguous()
    s = torch.empty((logits.shape[0],), dtype=torch.float32, device=logits.device)
    launch("runia_gen_score_f32", logits.data_ptr(), s.data_ptr(), logits.shape[0], logits.shape[1], int(m), float(gamma))
    return s


@_device_guard()
def proj_norm(x: torch.Tensor, u: torch.Tensor, packed_ns: torch.Tensor, n: int) -> torch.Tensor:
    """|| (x - u) @ NS ||_2 per row -> [N] f64 (x, u both f32 or both f64)."""
    require_gpu()
    assert x.is_cuda and x.dim() == 2 and x.dtype == u.dtype and x.dtype in (torch.float32, torch.float64)
    x, u = x.contiguous(), u.contiguous()
    nrow, d = x.shape
    out = torch.empty((nrow,), dtype=torch.float64, device=x.device)
    launch("runia_proj_norm_f32" if x.dtype == torch.float32 else "runia_proj_norm_f64", x.data_ptr(), u.data_ptr(),
           packed_ns.data_ptr(), out.data_ptr(), nrow, d, int(n))
    return out


@_device_guard()
def proj_sq_score(h: torch.Tensor, packed_m: torch.Tensor, c: torch.Tensor, r: int, out: Optional[torch.Tensor] = None,
                  trap: bool = False, balanced: bool = False) -> torch.Tensor:
    """score [N] = -|| M h + c ||^2 (h [N, D] f64, packed_m = pack(M.T), c [r]).  ``trap``: M is upper-trapezoidal
    (``qr_trapezoid``); the launch skips its zero blocks (``runia_proj_sq_score_trap_f64``).  ``balanced`` (with ``trap``):
    its row blocks stand in the balanced order (``trap_balance_rows``; ``runia_proj_sq_score_btrap_f64``)."""
    lib = load_library()
    require_gpu()
    assert h.is_cuda and h.dtype == torch.float64 and h.dim() == 2
    h = h.contiguous()
    nrow, d = h.shape
    s = torch.empty((nrow,), dtype=torch.float64, device=h.device) if out is None else out
    ws_bytes = int(lib.runia_proj_sq_workspace_bytes(nrow))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=h.device)
    launch(_proj_sq_entry("score", trap, balanced), h.data_ptr(), packed_m.data_ptr(),
           c.data_ptr(), s.data_ptr(), ws.data_ptr(), ws_bytes, nrow, d, int(r))
    return s


@_device_guard()
def qr_trapezoid(m: torch.Tensor, c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """m [r, D] f64 (r <= D), c [r] -> (R, Q c) with R = Q m upper-trapezoidal (``R[j, k]`` exactly 0 for k < j), Q orthogonal:
    ``|| R h + Q c || = || m h + c ||``.  Householder reflections in one workgroup, every sum in a fixed order
    (``runia_qr_trapezoid_f64``): equal input, equal bits."""
    require_gpu()
    assert m.is_cuda and m.dtype == torch.float64 and m.dim() == 2 and m.shape[0] <= m.shape[1]
    assert c.is_cuda and c.dtype == torch.float64 and c.shape == (m.shape[0],)
    m, c = m.contiguous(), c.contiguous()
    r_out, c_out = torch.empty_like(m), torch.empty_like(c)
    launch("runia_qr_trapezoid_f64", m.data_ptr(), c.data_ptr(), r_out.data_ptr(), c_out.data_ptr(), m.shape[0], m.shape[1])
    return r_out, c_out


def trap_balance_order(r: int) -> np.ndarray:
    """[r] int64: the row of an upper-trapezoidal R that stands at each row of its balanced form (``runia_trap_balance_order``,
    the rule of ``csrc/trap_order.hpp``; identity for r < 256 and on a last partial block of 256).  Host only: no GPU needed."""
    idx = np.empty(int(r), dtype=np.int64)
    call("runia_trap_balance_order", idx.ctypes.data, int(r))
    return idx


@_device_guard()
def trap_balance_rows(m: torch.Tensor, c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """m [r, D] f64 upper-trapezoidal (``qr_trapezoid``), c [r] -> both with their rows in the balanced order of
    ``trap_balance_order`` (``runia_trap_balance_rows_f64``): the same score, and the two column halves of K2' skip equally
    many chunks (``proj_sq_score(..., trap=True, balanced=True)``)."""
    require_gpu()
    assert m.is_cuda and m.dtype == torch.float64 and m.dim() == 2 and m.shape[0] <= m.shape[1]
    assert c.is_cuda and c.dtype == torch.float64 and c.shape == (m.shape[0],)
    m, c = m.contiguous(), c.contiguous()
    m_out, c_out = torch.empty_like(m), torch.empty_like(c)
    launch("runia_trap_balance_rows_f64", m.data_ptr(), c.data_ptr(), m_out.data_ptr(), c_out.data_ptr(), m.shape[0], m.shape[1])
    return m_out, c_out


def _ood_metrics_buffers(n: int, device):
    """The workspace of a runia_ood_metrics_* / runia_ood_clf_curve_* call over n scores, and its [3] f64 result:
    ``(ws, ws_ptr, ws_bytes, out)`` - ``ws`` owns the memory, ``ws_ptr`` is its first 256-byte aligned address."""
    ws_bytes = query("runia_ood_metrics_workspace_bytes", n)
    ws = workspace(ws_bytes + 256, device, 0)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, ws_bytes, torch.empty(3, dtype=torch.float64, device=device)


@_device_guard()
def ood_metrics(ind_scores: torch.Tensor, ood_scores: torch.Tensor) -> torch.Tensor:
    """Device scores (both f32 or both f64) -> device tensor [3] f64 = (auroc, fpr@95, aupr), InD = positive class
    (``get_auroc_results`` of the reference, evaluation/metrics.py:37-100).  Stream-ordered, no synchronisation."""
    require_gpu()
    assert ind_scores.is_cuda and ood_scores.is_cuda and ind_scores.dtype == ood_scores.dtype
    assert ind_scores.dtype in (torch.float32, torch.float64)
    a, b = ind_scores.reshape(-1).contiguous(), ood_scores.reshape(-1).contiguous()
    n = a.numel() + b.numel()
    ws, ws_ptr, ws_bytes, out = _ood_metrics_buffers(n, a.device)
    launch("runia_ood_metrics_f64" if a.dtype == torch.float64 else "runia_ood_metrics_f32", a.data_ptr(), a.numel(),
           b.data_ptr(), b.numel(), out.data_ptr(), ws_ptr, ws_bytes)
    return out


@_device_guard()
def ood_clf_curve(ind_scores: torch.Tensor, ood_scores: torch.Tensor):
    """Device scores (both f32 or both f64) -> ``(metrics [3] f64 device, tps [runs] int64 host, fps [runs] int64 host)``:
    torchmetrics' ``_binary_clf_curve`` (cumulative true / false positives at the end of every run of equal scores,
    descending) from the device sort + scans; only the compacted curve leaves the device (one synchronisation)."""
    require_gpu()
    assert ind_scores.is_cuda and ood_scores.is_cuda and ind_scores.dtype == ood_scores.dtype
    assert ind_scores.dtype in (torch.float32, torch.float64)
    a, b = ind_scores.reshape(-1).contiguous(), ood_scores.reshape(-1).contiguous()
    n = a.numel() + b.numel()
    ws, ws_ptr, ws_bytes, out = _ood_metrics_buffers(n, a.device)
    curve = torch.empty((2, n), dtype=torch.int32, device=a.device)  # u32 counts < 2^31 (n is limited to 2^31 - 1)
    n_points = torch.zeros(1, dtype=torch.int64, device=a.device)
    launch("runia_ood_clf_curve_f64" if a.dtype == torch.float64 else "runia_ood_clf_curve_f32", a.data_ptr(), a.numel(),
           b.data_ptr(), b.numel(), out.data_ptr(), curve[0].data_ptr(), curve[1].data_ptr(), n_points.data_ptr(), ws_ptr,
           ws_bytes)
    m = int(n_points.item())
    host = to_host(curve[:, :m].contiguous()).astype(np.int64)
    return out, host[0], host[1]


def boot_tile_rows() -> int:
    """Rows of one tile of the bootstrap walk (``runia_boot_tile_rows``; a host query)."""
    return query("runia_boot_tile_rows")


def boot_weights_host(seed: int, first_replicate: int, n_boot: int, ids) -> np.ndarray:
    """The Poisson(1) bootstrap weights ``[n_boot, len(ids)]`` uint8 of the replicates ``first_replicate ...`` for the row or
    group ids ``ids`` (``runia_boot_weights_host``): plain host code over the kernel's weight function, no GPU touched."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).astype(np.int32))
    out = np.empty((int(n_boot), ids.size), dtype=np.uint8)
    call("runia_boot_weights_host", int(seed) & (2**64 - 1), int(first_replicate), int(n_boot), ids.ctypes.data, ids.size,
         out.ctypes.data)
    return out


class BootOrder(NamedTuple):
    """A score table ordered for :func:`boot_metrics`: ``keys`` int64 [n] ascending (= descending score), ``rows`` int32 [n] the
    row of every key (InD rows first), ``n_ind``, and ``squashed`` [1] (device) - whether the scores went through the sigmoid."""

    keys: torch.Tensor
    rows: torch.Tensor
    n_ind: int
    squashed: torch.Tensor


@_device_guard()
def boot_order(ind_scores: torch.Tensor, ood_scores: torch.Tensor) -> BootOrder:
    """Device scores (both f32 or both f64) -> their :class:`BootOrder`: the metrics step's keys (``runia_boot_keys_*``) and one
    stable device sort of them - once per method, whatever the number of replicates."""
    require_gpu()
    if not (isinstance(ind_scores, torch.Tensor) and isinstance(ood_scores, torch.Tensor) and ind_scores.is_cuda and ood_scores.is_cuda):
        raise RuniaHipError("boot_order: scores must be device tensors")
    if ind_scores.dtype != ood_scores.dtype or ind_scores.dtype not in (torch.float32, torch.float64):
        raise RuniaHipError("boot_order: scores must both be float32 or both float64")
    a, b = ind_scores.reshape(-1).contiguous(), ood_scores.reshape(-1).contiguous()
    if a.numel() < 1 or b.numel() < 1:
        raise RuniaHipError("boot_order: n_ind >= 1 and n_ood >= 1 are required")
    n = a.numel() + b.numel()
    keys = torch.empty(n, dtype=torch.int64, device=a.device)
    flag = torch.empty(1, dtype=torch.int32, device=a.device)
    launch("runia_boot_keys_f64" if a.dtype == torch.float64 else "runia_boot_keys_f32", a.data_ptr(), a.numel(), b.data_ptr(),
           b.numel(), keys.data_ptr(), flag.data_ptr())
    skeys, order = torch.sort(keys, stable=True)
    return BootOrder(skeys, order.to(torch.int32), a.numel(), flag)


@_device_guard()
def boot_metrics(order: BootOrder, n_boot: int, seed: int = 0, first_replicate: int = 0,
                 group_of_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(AUROC, FPR@95, AUPR)`` of the Poisson-bootstrap replicates ``first_replicate .. first_replicate + n_boot - 1`` of an
    ordered score table -> device tensor ``[n_boot, 3]`` f64 (``runia_boot_metrics``; NaN rows: replicates in which one side drew
    nothing).  ``group_of_row`` int32 ``[n]``: resample by group.  Stream-ordered, no synchronisation."""
    require_gpu()
    keys, rows, n_ind = order.keys, order.rows, int(order.n_ind)
    n, n_boot, first_replicate = keys.numel(), int(n_boot), int(first_replicate)
    if not (keys.is_cuda and rows.is_cuda and keys.dtype == torch.int64 and rows.dtype == torch.int32):
        raise RuniaHipError("boot_metrics: keys must be int64 and rows int32 device tensors")
    if not (keys.is_contiguous() and rows.is_contiguous() and rows.numel() == n and rows.device == keys.device):
        raise RuniaHipError("boot_metrics: keys and rows must be contiguous, of one length, on one device")
    if n_ind < 1 or n - n_ind < 1:
        raise RuniaHipError("boot_metrics: n_ind >= 1 and n_ood >= 1 are required")
    if n_boot < 1 or first_replicate < 0:
        raise RuniaHipError("boot_metrics: n_boot >= 1 and first_replicate >= 0 are required")
    if group_of_row is not None:
        if not (group_of_row.is_cuda and group_of_row.dtype == torch.int32 and group_of_row.is_contiguous()
                and group_of_row.numel() == n and group_of_row.device == keys.device):
            raise RuniaHipError("boot_metrics: group_of_row must be a contiguous int32 device tensor with one entry per row")
    out = torch.empty((n_boot, 3), dtype=torch.float64, device=keys.device)
    ws_bytes = query("runia_boot_workspace_bytes", n, n_boot)
    ws = workspace(ws_bytes, keys.device)
    launch("runia_boot_metrics", keys.data_ptr(), rows.data_ptr(), n, n_ind, _ptr(group_of_row), int(seed) & (2**64 - 1),
           first_replicate, n_boot, out.data_ptr(), ws.data_ptr(), ws_bytes)
    return out


def sel_tile_rows() -> int:
    """Rows of one tile of the selective-prediction scan (``runia_sel_tile_rows``; a host query)."""
    return query("runia_sel_tile_rows")


def sel_key_of_host(confidence: float) -> int:
    """The sort key ``runia_sel_keys_*`` gives one confidence (``runia_sel_key_of_f64_host``: plain host code, no GPU touched)."""
    return query("runia_sel_key_of_f64_host", float(confidence))


ORDER_FORMS = {f: _HEADER_MACROS["RUNIA_ORDER_" + f.upper()]
               for f in ("asc", "desc", "asc_fold", "desc_fold", "desc_one_nan", "desc_signed", "asc_nonneg")}


def order_keys_host(values: np.ndarray, form: str) -> Tuple[np.ndarray, np.ndarray]:
    """``(keys uint64 [n], back [n])``: the ordered key of csrc/order.hpp of every float32 / float64 value under one of
    :data:`ORDER_FORMS`, and the inverse of every key in the values' dtype (``runia_order_keys_host``: plain host code over the
    kernels' header, no GPU touched)."""
    v = np.ascontiguousarray(values)
    assert v.ndim == 1 and v.dtype in (np.float32, np.float64), "values: a 1-D float32 or float64 array"
    keys, back = np.empty(v.shape, dtype=np.uint64), np.empty_like(v)
    call("runia_order_keys_host", v.ctypes.data, v.size, int(v.dtype == np.float64), ORDER_FORMS[form], keys.ctypes.data,
         back.ctypes.data)
    return keys, back


class SelOrder(NamedTuple):
    """A confidence table ordered for :func:`sel_curve`: ``keys`` int64 [n] ascending (= descending confidence), ``rows`` int32 [n]
    the row of every key - the shape of :class:`BootOrder` - and ``bad`` [1] (device): whether any confidence is NaN."""

    keys: torch.Tensor
    rows: torch.Tensor
    bad: torch.Tensor


class SelCurve(NamedTuple):
    """What :func:`sel_curve` leaves on the device: ``record`` f64 [5] = (n_points, L_n, S_n, aurc, augrc); the compacted curve
    ``run_end`` int32 / ``cum_loss`` / ``cum_conf`` f64, allocated for ``n`` points with the first ``n_points`` [1] int64 (device)
    filled, or three ``None`` when it was not asked for."""

    record: torch.Tensor
    run_end: Optional[torch.Tensor]
    cum_loss: Optional[torch.Tensor]
    cum_conf: Optional[torch.Tensor]
    n_points: torch.Tensor
    n: int


def _sel_vector(name: str, what: str, t, n: Optional[int] = None) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuniaHipError(f"{name}: {what} must be a device tensor")
    if t.dtype not in (torch.float32, torch.float64):
        raise RuniaHipError(f"{name}: {what} must be float32 or float64, got {t.dtype}")
    if t.dim() != 1 or t.numel() < 1 or t.numel() >= 2**31 or (n is not None and t.numel() != n):
        raise RuniaHipError(f"{name}: {what} must be a vector of {'1 .. 2^31 - 1' if n is None else n} entries, got shape "
                            f"{tuple(t.shape)}")
    return t.contiguous()


@_device_guard()
def sel_order(confidence: torch.Tensor) -> SelOrder:
    """Device confidences [n] (f32 or f64) -> their :class:`SelOrder`: the keys of ``runia_sel_keys_*`` and one stable device sort
    of them (plumbing, as in :func:`boot_order`)."""
    require_gpu()
    conf = _sel_vector("sel_order", "confidence", confidence)
    n = conf.numel()
    keys = torch.empty(n, dtype=torch.int64, device=conf.device)
    bad = torch.empty(1, dtype=torch.int32, device=conf.device)
    launch("runia_sel_keys_f64" if conf.dtype == torch.float64 else "runia_sel_keys_f32", conf.data_ptr(), n, keys.data_ptr(),
           bad.data_ptr())
    skeys, order = torch.sort(keys, stable=True)
    return SelOrder(skeys, order.to(torch.int32), bad)


@_device_guard()
def sel_curve(order: SelOrder, loss: torch.Tensor, want_curve: bool = True) -> SelCurve:
    """The risk-coverage scan of an ordered table (``runia_sel_curve``): ``loss`` [n] (f32 or f64) is read through ``order.rows``;
    the confidences come back out of the keys.  Stream-ordered, no synchronisation.  The same inputs give the same bits; with
    integer-valued losses any permutation of the rows does."""
    require_gpu()
    keys, rows = order.keys, order.rows
    if not (isinstance(keys, torch.Tensor) and isinstance(rows, torch.Tensor) and keys.is_cuda and rows.is_cuda
            and keys.dtype == torch.int64 and rows.dtype == torch.int32):
        raise RuniaHipError("sel_curve: keys must be int64 and rows int32 device tensors")
    n = keys.numel()
    if not (keys.dim() == 1 and keys.is_contiguous() and rows.is_contiguous() and rows.shape == keys.shape and 1 <= n < 2**31):
        raise RuniaHipError("sel_curve: keys and rows must be contiguous vectors of one length in 1 .. 2^31 - 1")
    loss = _sel_vector("sel_curve", "loss", loss, n)
    dev = keys.device
    record = torch.empty(5, dtype=torch.float64, device=dev)
    n_points = torch.empty(1, dtype=torch.int64, device=dev)
    run_end = torch.empty(n, dtype=torch.int32, device=dev) if want_curve else None
    cum_loss = torch.empty(n, dtype=torch.float64, device=dev) if want_curve else None
    cum_conf = torch.empty(n, dtype=torch.float64, device=dev) if want_curve else None
    ws_bytes = query("runia_sel_workspace_bytes", n)
    ws = workspace(ws_bytes, dev)
    launch("runia_sel_curve", keys.data_ptr(), rows.data_ptr(), loss.data_ptr(), int(loss.dtype == torch.float64), n,
           record.data_ptr(), _ptr(run_end), _ptr(cum_loss), _ptr(cum_conf), n_points.data_ptr(), ws.data_ptr(), ws_bytes)
    return SelCurve(record, run_end, cum_loss, cum_conf, n_points, n)


@_device_guard()
def sel_query(curve: SelCurve, targets=(), risks=(), n_bins: int = 0):
    """Queries on a compacted curve (``runia_sel_query``): ``targets`` - the integers ``k_c = ceil(c n)`` of at most 64 coverage
    targets; ``risks`` - at most 64 risk levels; ``n_bins`` in 0 .. 512 equal-mass bins.  -> device tensors ``(risk_at [Q],
    coverage_at [Q], coverage_at_risk [R], bins [n_bins, 3])`` f64 (``bins``: count, loss sum, confidence sum, least confident
    bin first).  Stream-ordered, no synchronisation."""
    require_gpu()
    targets = [int(k) for k in targets]
    risks = [float(r) for r in risks]
    n_bins, n = int(n_bins), int(curve.n)
    if len(targets) > 64 or len(risks) > 64:
        raise RuniaHipError("sel_query: at most 64 coverage targets and 64 risk levels")
    if not 0 <= n_bins <= 512:
        raise RuniaHipError("sel_query: n_bins must lie in 0 .. 512")
    if any(k < 1 or k > n for k in targets):
        raise RuniaHipError(f"sel_query: coverage targets must lie in 1 .. n = {n}")
    if curve.run_end is None:
        raise RuniaHipError("sel_query: the curve was not kept (sel_curve(..., want_curve=True))")
    for name, t, dt in (("run_end", curve.run_end, torch.int32), ("cum_loss", curve.cum_loss, torch.float64),
                        ("cum_conf", curve.cum_conf, torch.float64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= n
                and t.device == curve.n_points.device):
            raise RuniaHipError(f"sel_query: {name} must be a contiguous {dt} device tensor of n = {n} entries")
    if not (curve.n_points.is_cuda and curve.n_points.dtype == torch.int64 and curve.n_points.numel() == 1):
        raise RuniaHipError("sel_query: n_points must be one int64 on the device")
    dev = curve.n_points.device
    q, r = len(targets), len(risks)
    tg = torch.tensor(targets, dtype=torch.int64).to(dev) if q else None
    rk = torch.tensor(risks, dtype=torch.float64).to(dev) if r else None
    out = torch.empty(2 * q + r + 3 * n_bins, dtype=torch.float64, device=dev)
    risk_at, cov_at, cov_risk, bins = out[:q], out[q:2 * q], out[2 * q:2 * q + r], out[2 * q + r:].view(n_bins, 3)
    ws = workspace(256, dev, 256)
    launch("runia_sel_query", curve.run_end.data_ptr(), curve.cum_loss.data_ptr(), curve.cum_conf.data_ptr(),
           curve.n_points.data_ptr(), n, _ptr(tg), q, _ptr(rk), r, n_bins, risk_at.data_ptr() if q else None,
           cov_at.data_ptr() if q else None, cov_risk.data_ptr() if r else None, bins.data_ptr() if n_bins else None,
           ws.data_ptr(), 256)
    return risk_at, cov_at, cov_risk, bins


def boot_sel_tile_rows() -> int:
    """Rows of one tile of the selective bootstrap walk (``runia_boot_sel_tile_rows``; a host query)."""
    return query("runia_boot_sel_tile_rows")


@_device_guard()
def boot_sel_metrics(order: SelOrder, loss: torch.Tensor, n_boot: int, seed: int = 0, first_replicate: int = 0,
                     group_of_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(aurc, augrc, risk, n')`` of the Poisson-bootstrap replicates ``first_replicate .. first_replicate + n_boot - 1`` of an
    ordered confidence table -> device tensor ``[n_boot, 4]`` f64 (``runia_boot_sel_metrics``; three NaN where a replicate drew
    nothing).  ``loss`` [n] (f32 or f64, finite) is read through ``order.rows``; ``group_of_row`` int32 ``[n]``: resample by
    group.  The weights are those of :func:`boot_metrics` for the same ids.  Stream-ordered, no synchronisation."""
    require_gpu()
    keys, rows = order.keys, order.rows
    if not (isinstance(keys, torch.Tensor) and isinstance(rows, torch.Tensor) and keys.is_cuda and rows.is_cuda
            and keys.dtype == torch.int64 and rows.dtype == torch.int32):
        raise RuniaHipError("boot_sel_metrics: keys must be int64 and rows int32 device tensors")
    n, n_boot, first_replicate = keys.numel(), int(n_boot), int(first_replicate)
    if not (keys.dim() == 1 and keys.is_contiguous() and rows.is_contiguous() and rows.shape == keys.shape
            and rows.device == keys.device and 1 <= n < 2**31):
        raise RuniaHipError("boot_sel_metrics: keys and rows must be contiguous vectors of one length in 1 .. 2^31 - 1")
    loss = _sel_vector("boot_sel_metrics", "loss", loss, n)
    if loss.device != keys.device:
        raise RuniaHipError("boot_sel_metrics: loss must lie on the device of the ordered table")
    if n_boot < 1 or first_replicate < 0:
        raise RuniaHipError("boot_sel_metrics: n_boot >= 1 and first_replicate >= 0 are required")
    if group_of_row is not None:
        if not (group_of_row.is_cuda and group_of_row.dtype == torch.int32 and group_of_row.is_contiguous()
                and group_of_row.numel() == n and group_of_row.device == keys.device):
            raise RuniaHipError("boot_sel_metrics: group_of_row must be a contiguous int32 device tensor with one entry per row")
    out = torch.empty((n_boot, 4), dtype=torch.float64, device=keys.device)
    launch("runia_boot_sel_metrics", keys.data_ptr(), rows.data_ptr(), loss.data_ptr(), int(loss.dtype == torch.float64), n,
           _ptr(group_of_row), int(seed) & (2**64 - 1), first_replicate, n_boot, out.data_ptr())
    return out


SHIFT_KERNELS = {"rbf": 0, "energy": 1, "linear": 2}     # `kind` of runia_shift_mmd
SHIFT_ESTIMATORS = {"biased": 0, "unbiased": 1}          # `estimator` of runia_shift_mmd
SHIFT_MAX_ROWS = 1 << 18                                 # pooled rows of one test (the row index shares a key with the word)
SHIFT_MAX_BANDWIDTHS = 8


class ShiftSums(NamedTuple):
    """Outputs of :func:`shift_mmd`, all on the device: ``t``, ``u``, ``stats`` f64 ``[1 + n_perm]`` (entry 0: the observed split),
    ``S`` f64 ``[1]``, ``count`` int64 ``[1]``, ``p_value`` f64 ``[1]``."""

    t: torch.Tensor
    u: torch.Tensor
    S: torch.Tensor
    stats: torch.Tensor
    count: torch.Tensor
    p_value: torch.Tensor


def _shift_perm_args(n: int, N: int, first_perm: int, n_rows: int):
    n, N, first_perm, n_rows = int(n), int(N), int(first_perm), int(n_rows)
    if not (1 <= n < N <= SHIFT_MAX_ROWS) or first_perm < 0 or n_rows < 1:
        raise RuniaHipError("shift_perm_bits: 1 <= n < N <= 2^18, first_perm >= 0 and n_rows >= 1 are required")
    return n, N, first_perm, n_rows, (N + 31) // 32


def shift_perm_bits_host(seed: int, n: int, N: int, first_perm: int, n_rows: int) -> np.ndarray:
    """Rows ``first_perm ...`` of the membership table of the two-sample tests as packed bits, uint32 ``[n_rows, ceil(N / 32)]``
    (``runia_shift_perm_bits_host``): plain host code over the kernel's key function, no GPU touched."""
    n, N, first_perm, n_rows, words = _shift_perm_args(n, N, first_perm, n_rows)
    out = np.empty((n_rows, words), dtype=np.uint32)
    call("runia_shift_perm_bits_host", int(seed) & (2**64 - 1), n, N, first_perm, n_rows, out.ctypes.data, words)
    return out


def shift_perm_bits(seed: int, n: int, N: int, first_perm: int, n_rows: int) -> torch.Tensor:
    """The same table from the membership kernel (``runia_shift_perm_bits``): device tensor int32 ``[n_rows, ceil(N / 32)]`` holding
    the uint32 words."""
    n, N, first_perm, n_rows, words = _shift_perm_args(n, N, first_perm, n_rows)
    dev = require_gpu()
    out = torch.empty((n_rows, words), dtype=torch.int32, device=dev)
    launch("runia_shift_perm_bits", int(seed) & (2**64 - 1), n, N, first_perm, n_rows, out.data_ptr(), words)
    return out


def _shift_rows(name: str, x: torch.Tensor, y: torch.Tensor):
    """Two device row tables of one dtype (f32 / f16 / bf16) and width, each with unit column stride (row views are read in place)."""
    for t in (x, y):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in ELEM_DTYPE_CODES):
            raise RuniaHipError(f"{name}: rows must be 2-D float32, float16 or bfloat16 device tensors")
    if x.dtype != y.dtype or x.shape[1] != y.shape[1] or x.device != y.device:
        raise RuniaHipError(f"{name}: the two tables must share dtype, width and device")
    if x.shape[0] < 1 or y.shape[0] < 1 or x.shape[1] < 1 or x.shape[0] + y.shape[0] > SHIFT_MAX_ROWS:
        raise RuniaHipError(f"{name}: n, m, D >= 1 and n + m <= 2^18 are required")

    def rows_in_place(t):
        return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) or t.shape[0] == 1 and t.stride(1) == 1 else t.contiguous()

    return rows_in_place(x), rows_in_place(y)


@_device_guard()
def shift_pairwise_sample(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Distances between the rows of the bandwidth sample of the pooled table ``[x; y]`` (``runia_shift_pairwise_sample``): the
    upper triangle, f32 ``[M (M - 1) / 2]``, of the ``M = min(N, 2048)`` pooled rows ``floor(k N / M)``."""
    require_gpu()
    x, y = _shift_rows("shift_pairwise_sample", x, y)
    m_rows = query("runia_shift_sample_rows", x.shape[0] + y.shape[0])
    out = torch.empty((m_rows * (m_rows - 1) // 2,), dtype=torch.float32, device=x.device)
    launch("runia_shift_pairwise_sample", x.data_ptr(), x.shape[0], max(x.stride(0), x.shape[1]), y.data_ptr(), y.shape[0],
           max(y.stride(0), y.shape[1]), x.shape[1], ELEM_DTYPE_CODES[x.dtype], out.data_ptr())
    return out


@_device_guard()
def shift_mmd(x: torch.Tensor, y: torch.Tensor, kernel: str, bandwidths, estimator: str, n_perm: int, seed: int = 0,
              kernel_events: Optional[list] = None) -> ShiftSums:
    """The kernel two-sample sums and statistics of ``x`` [n, D] against ``y`` [m, D] under the observed split and ``n_perm``
    permutations (``runia_shift_mmd``) -> :class:`ShiftSums`.  ``bandwidths``: the sigmas of the rbf kernel (host numbers, 1 .. 8 of
    them), ignored by the other kernels.  Stream-ordered, no synchronisation; the same bits from call to call.  ``kernel_events``: a
    list that receives the event pair of the call's first fused-kernel launch (its own start / end timestamps)."""
    require_gpu()
    x, y = _shift_rows("shift_mmd", x, y)
    if kernel not in SHIFT_KERNELS or estimator not in SHIFT_ESTIMATORS:
        raise RuniaHipError(f"shift_mmd: kernel must be one of {sorted(SHIFT_KERNELS)} and estimator of {sorted(SHIFT_ESTIMATORS)}")
    n, m, d, n_perm = x.shape[0], y.shape[0], x.shape[1], int(n_perm)
    bw = np.ascontiguousarray(np.atleast_1d(np.asarray(bandwidths if kernel == "rbf" else [1.0], dtype=np.float64)))
    if n_perm < 1 or bw.ndim != 1 or not (1 <= bw.size <= SHIFT_MAX_BANDWIDTHS):
        raise RuniaHipError("shift_mmd: n_perm >= 1 and 1 .. 8 bandwidths are required")
    p = 1 + n_perm
    f64 = dict(dtype=torch.float64, device=x.device)
    out = ShiftSums(torch.empty(p, **f64), torch.empty(p, **f64), torch.empty(1, **f64), torch.empty(p, **f64),
                    torch.empty(1, dtype=torch.int64, device=x.device), torch.empty(1, **f64))
    ws_bytes = query("runia_shift_workspace_bytes", n, m, d, n_perm)
    ws = workspace(ws_bytes, x.device)
    args = (x.data_ptr(), n, max(x.stride(0), d), y.data_ptr(), m, max(y.stride(0), d), d, ELEM_DTYPE_CODES[x.dtype],
            SHIFT_KERNELS[kernel], bw.ctypes.data, int(bw.size), SHIFT_ESTIMATORS[estimator], int(seed) & (2**64 - 1), n_perm,
            out.t.data_ptr(), out.u.data_ptr(), out.S.data_ptr(), out.stats.data_ptr(), out.count.data_ptr(), out.p_value.data_ptr(),
            ws.data_ptr(), ws_bytes)
    if kernel_events is not None:
        kernel_events.append(_timed_call("runia_shift_mmd", *args))
    else:
        launch("runia_shift_mmd", *args)
    return out


KS_MAX_PERM = (1 << 20) - 1                              # permutations of one runia_ks_perm_table call


def ks_max_rows() -> int:
    """The largest pooled ``n + m`` of one :func:`ks_perm_table` call (``runia_ks_max_rows``); needs no GPU."""
    return query("runia_ks_max_rows")


@_device_guard()
def ks_perm_table(x: torch.Tensor, y: torch.Tensor, n_perm: int, seed: int = 0, kernel_events: Optional[list] = None):
    """The integer Kolmogorov-Smirnov table of ``x`` [n, D] against ``y`` [m, D] (``runia_ks_perm_table``) -> ``(table, valid)``:
    ``table`` int64 ``[1 + n_perm, D]``, row 0 the observed split and row p the permutation p of :func:`shift_perm_bits`, each
    entry ``n m`` times the two-sample KS statistic of that column (``-1`` in a column that holds a NaN); ``valid`` int32 ``[D]``.
    Rows are read in place as in :func:`shift_mmd`.  Stream-ordered, no synchronisation; the same bits from call to call.
    ``kernel_events`` is a measurement hook for ``tools/ablate/run_shift_ks.py``, not part of the scoring interface: a list that
    receives the event pair of the call's first walk-kernel launch (its own start / end timestamps)."""
    require_gpu()
    x, y = _shift_rows("ks_perm_table", x, y)
    n, m, d, n_perm = x.shape[0], y.shape[0], x.shape[1], int(n_perm)
    if n + m > ks_max_rows() or not (0 <= n_perm <= KS_MAX_PERM):
        raise RuniaHipError(f"ks_perm_table: n + m <= {ks_max_rows()} and 0 <= n_perm < 2^20 are required")
    table = torch.empty((1 + n_perm, d), dtype=torch.int64, device=x.device)
    valid = torch.empty((d,), dtype=torch.int32, device=x.device)
    ws_bytes = query("runia_ks_workspace_bytes", n, m, d, n_perm)
    ws = workspace(ws_bytes, x.device)
    args = (x.data_ptr(), n, max(x.stride(0), d), y.data_ptr(), m, max(y.stride(0), d), d, ELEM_DTYPE_CODES[x.dtype],
            int(seed) & (2**64 - 1), n_perm, table.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws_bytes)
    if kernel_events is not None:
        kernel_events.append(_timed_call("runia_ks_perm_table", *args))
    else:
        launch("runia_ks_perm_table", *args)
    return table, valid


@_device_guard()
def eigh(a: torch.Tensor, max_sweeps: int = 30, blocked: bool = True, info: Optional[dict] = None):
    """Symmetric eigen-decomposition on the device: a [n, n] f64 -> (eigenvalues [n] ascending, eigenvectors [n, n] as
    columns), like ``numpy.linalg.eigh``.  Cyclic Jacobi sweeps until one applies no rotation; ``blocked`` (default):
    ``runia_eigh_block_sweep_f64`` - 64 x 64 sub-problems in LDS + matrix-core updates, (n/32 - 1) x 2 launches per sweep;
    ``blocked=False``: the scalar-rotation form ``runia_eigh_sweep_f64`` (2 (n - 1) launches per sweep).
    Setup-time: reads one counter back per sweep.  ``info`` (optional dict) receives ``sweeps`` and ``rotations``.

    Non-finite input: when the Frobenius norm of ``a`` is not finite in f64 (a NaN or an infinite entry, or entries above
    ~1e154 whose squares overflow) EVERY returned eigenvalue is NaN and the eigenvectors mean nothing.  The sweeps are
    bounded by ``max_sweeps`` on the host, so the call returns (both forms stop rotating once the NaN has spread over the
    matrix; an infinite norm makes every rotation threshold infinite, so no rotation is applied at all and the diagonal
    left behind is not a spectrum) or raises ``RuniaHipError`` like any matrix that has not settled."""
    require_gpu()
    assert a.is_cuda and a.dtype == torch.float64 and a.dim() == 2 and a.shape[0] == a.shape[1]
    n = a.shape[0]
    sym = (a + a.T) * 0.5  # exactly symmetric input
    count = torch.zeros(1, dtype=torch.int32, device=a.device)
    if blocked:
        big = query("runia_eigh_block_padded", n)
        work = torch.zeros((big, big), dtype=torch.float64, device=a.device)
        work[:n, :n] = sym
        ws_bytes = query("runia_eigh_block_workspace_bytes", n)
        init, sweep, size = "runia_eigh_block_init_f64", "runia_eigh_block_sweep_f64", big
    else:
        work = sym.contiguous()
        ws_bytes = query("runia_eigh_workspace_bytes", n)
        init, sweep, size = "runia_eigh_init_f64", "runia_eigh_sweep_f64", n
    v = torch.empty_like(work)
    ws = workspace(ws_bytes + 16, a.device, 0)
    off = (-ws.data_ptr()) % 16
    launch(init, work.data_ptr(), v.data_ptr(), size, ws.data_ptr() + off, ws_bytes)
    done = 0
    for sweep_no in range(1, max_sweeps + 1):
        launch(sweep, work.data_ptr(), v.data_ptr(), size, ws.data_ptr() + off, ws_bytes, count.data_ptr())
        total = int(count.item())
        if total == done:
            break
        done = total
    else:
        raise RuniaHipError(f"the Jacobi sweeps did not converge in {max_sweeps} sweeps (n = {n})")
    if info is not None:
        info["sweeps"] = info.get("sweeps", 0) + sweep_no
        info["rotations"] = info.get("rotations", 0) + done
        info["calls"] = info.get("calls", 0) + 1
    anorm = ws[off:off + 8].view(torch.float64)  # what the init kernel left: the norm that scales the rotation threshold
    w = torch.where(torch.isfinite(anorm), torch.diagonal(work)[:n], torch.full_like(anorm, float("nan")))
    # ascending order: n scalars, ranked on the host (the convergence loop has synchronised already; no device sort)
    order = torch.from_numpy(np.argsort(w.cpu().numpy(), kind="stable")).to(a.device)
    return w[order], v[:n, :n][:, order].contiguous()


@_device_guard()
def matmul_f64(a: torch.Tensor, b: torch.Tensor, transpose_b: bool = False) -> torch.Tensor:
    require_gpu()
    assert a.is_cuda and b.is_cuda and a.dtype == torch.float64 and b.dtype == torch.float64
    a, b = a.contiguous(), b.contiguous()
    m, k = a.shape
    n = b.shape[0] if transpose_b else b.shape[1]
    assert (b.shape[1] if transpose_b else b.shape[0]) == k
    c = torch.empty((m, n), dtype=torch.float64, device=a.device)
    launch("runia_matmul_f64", a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, 1 if transpose_b else 0)
    return c


@_device_guard()
def centred_gram(e: torch.Tensor, denom: float) -> torch.Tensor:
    """e [n, H] f32 -> Gram matrix [n, n] f64 of the column-centred rows, divided by ``denom``."""
    require_gpu()
    assert e.is_cuda and e.dtype == torch.float32 and e.dim() == 2
    e = e.contiguous()
    n, h = e.shape
    g = torch.empty((n, n), dtype=torch.float64, device=e.device)
    launch("runia_centred_gram_f32", e.data_ptr(), g.data_ptr(), n, h, float(denom))
    return g


EIGEN_SCORE_MAX_K = 64


@_device_guard()
def eigen_scores(e: torch.Tensor, k: int, alpha: float = 1e-3) -> torch.Tensor:
    """e [G * k, H] f32 / f16 / bf16 (host or one GPU, any row stride) -> [G] f64: the eigen_score of every group of k
    consecutive rows, all groups in ONE launch of ``runia_eigen_score_batch`` (2 <= k <= 64).  Device rows are read in place
    (a view whose columns are not unit-stride is made contiguous); host rows go up in one copy in their own dtype.  The
    result lies where ``e`` does."""
    load_library()  # a missing library is reported before any argument
    if not isinstance(e, torch.Tensor) or e.dim() != 2:
        raise ValueError("eigen_scores takes a 2-D (G * k, hidden) tensor")
    if e.dtype not in ELEM_DTYPE_CODES:
        raise TypeError(f"eigen_scores takes float32, float16 or bfloat16 rows, not {e.dtype}")
    n, h = (int(v) for v in e.shape)
    k = int(k)
    if not 2 <= k <= EIGEN_SCORE_MAX_K:
        raise ValueError(f"groups of k = {k} samples: the kernel takes 2 <= k <= {EIGEN_SCORE_MAX_K}")
    if n == 0 or h == 0 or n % k:
        raise ValueError(f"{n} rows of width {h} do not form groups of {k} samples")
    dev = require_gpu()
    on_host = not e.is_cuda
    x = e.detach()
    if on_host:
        x = x.contiguous().to(dev)
    elif h > 1 and x.stride(1) != 1:
        x = x.contiguous()
    out = torch.empty(n // k, dtype=torch.float64, device=x.device)
    launch("runia_eigen_score_batch", x.data_ptr(), ELEM_DTYPE_CODES[x.dtype], n // k, k, h, x.stride(0), float(alpha),
           out.data_ptr())
    return out.cpu() if on_host else out


CONS_MAX_K = _HEADER_MACROS["RUNIA_CONS_MAX_K"]
CONS_MAX_T = _HEADER_MACROS["RUNIA_CONS_MAX_T"]
CONS_MAX_EOS = _HEADER_MACROS["RUNIA_CONS_MAX_EOS"]
_CONS_LCS, _CONS_JACCARD = _HEADER_MACROS["RUNIA_CONS_LCS"], _HEADER_MACROS["RUNIA_CONS_JACCARD"]


@_device_guard()
def cons_pairs(ids: torch.Tensor, k: int, eos: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
               lcs: bool = True, jaccard: bool = True):
    """ids [G * k, T] int32 / int64 on the GPU (any strides, read in place), eos [n] int64 and lengths [G * k] int64 device
    tensors or None -> ``(len [G * k], lcs [G, k, k] | None, uniq [G * k] | None, inter [G, k, k] | None)`` int32 device
    tensors: one call of ``runia_cons_pairs``.  The arguments are checked by ``llm_uncertainty.consistency``."""
    require_gpu()
    assert ids.is_cuda and ids.dim() == 2 and ids.dtype in (torch.int32, torch.int64) and (lcs or jaccard)
    rows, t = (int(v) for v in ids.shape)
    g = rows // k
    what = (_CONS_LCS if lcs else 0) | (_CONS_JACCARD if jaccard else 0)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=ids.device)  # noqa: E731
    ln = i32(rows)
    lc = i32(g, k, k) if lcs else None
    uq, it = (i32(rows), i32(g, k, k)) if jaccard else (None, None)
    ws_bytes = query("runia_cons_pairs_workspace_bytes", g, k, t, what)
    ws = workspace(ws_bytes, ids.device)
    launch("runia_cons_pairs", ids.data_ptr(), ids.element_size(), g, k, t, ids.stride(0), ids.stride(1), _ptr(eos),
           0 if eos is None else int(eos.numel()), _ptr(lengths), what, ln.data_ptr(), _ptr(lc), _ptr(uq), _ptr(it),
           ws.data_ptr(), ws_bytes)
    return ln, lc, uq, it


@_device_guard()
def cons_graph(w: torch.Tensor, eigv_threshold: float, set_threshold: float):
    """w [G, k, k] f64 contiguous on the GPU -> ``(eigenvalues [G, k], u_deg, u_eigv, u_ecc, lexsim [G], c_deg, c_ecc [G, k]``
    f64, ``num_sets [G]`` int32): one launch of ``runia_cons_graph``."""
    require_gpu()
    assert w.is_cuda and w.dtype == torch.float64 and w.dim() == 3 and w.shape[1] == w.shape[2] and w.is_contiguous()
    g, k = int(w.shape[0]), int(w.shape[1])
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=w.device)  # noqa: E731
    lam, u_deg, u_eigv, u_ecc, lexsim, c_deg, c_ecc = f64(g, k), f64(g), f64(g), f64(g), f64(g), f64(g, k), f64(g, k)
    sets = torch.empty(g, dtype=torch.int32, device=w.device)
    launch("runia_cons_graph", w.data_ptr(), g, k, float(eigv_threshold), float(set_threshold), lam.data_ptr(),
           u_deg.data_ptr(), u_eigv.data_ptr(), u_ecc.data_ptr(), lexsim.data_ptr(), c_deg.data_ptr(), c_ecc.data_ptr(),
           sets.data_ptr())
    return lam, u_deg, u_eigv, u_ecc, lexsim, c_deg, c_ecc, sets


@_device_guard("boxes", "batch_idx")
def roi_align(x: torch.Tensor, boxes: torch.Tensor, output_size, spatial_scale: float = 1.0, sampling_ratio: int = -1,
              aligned: bool = False, batch_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``torchvision.ops.roi_align``: x [B, C, H, W] f32, boxes [K, 4] f32 (xyxy) -> [K, C, PH, PW] f32 (device)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    boxes = boxes.to(device=x.device, dtype=torch.float32).contiguous()
    b, c, h, w = x.shape
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    k = boxes.shape[0]
    if batch_idx is not None:
        batch_idx = batch_idx.to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty((k, c, ph, pw), dtype=torch.float32, device=x.device)
    launch("runia_roi_align_f32", x.data_ptr(), boxes.data_ptr(), _ptr(batch_idx), out.data_ptr(), k, b, c, h, w, int(ph),
           int(pw), float(spatial_scale), int(sampling_ratio), 1 if aligned else 0)
    return out


@_device_guard()
def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """x [B, C, H, W] f32 -> [B, H, W, C] f32 (a contiguous copy in channels-last order; the ROI source of
    :func:`roi_mc_entropy`: 64 channels of a wave read a bilinear tap as one contiguous run)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    launch("runia_nchw_to_nhwc_f32", x.data_ptr(), out.data_ptr(), b, c, h * w)
    return out


ROI_FUSED_MAX_IMAGE_BYTES = 1 << 30  # one image's feature map behind a 32-bit buffer, with room for the offsets of outside samples


def roi_mc_entropy_supported(ph: int, pw: int, n_mc: int, k: int, sampling_ratio: int) -> bool:
    return bool(query("runia_roi_mc_entropy_supported", int(ph), int(pw), int(n_mc), int(k), int(sampling_ratio)))


@_device_guard("boxes", "batch_idx", "rand")
def roi_mc_entropy(x_nhwc: torch.Tensor, boxes: torch.Tensor, output_size, spatial_scale: float, sampling_ratio: int,
                   aligned: bool, rand: Union[torch.Tensor, CounterDraws, None], n_mc: int, drop_prob: float, block_size: int, k: int,
                   min_dist: float = 1e-5, batch_idx: Optional[torch.Tensor] = None, return_samples: bool = False):
    """``roi_align`` -> per-ROI ``MCSamplerModule`` -> per-dimension entropy in ONE pass from the feature map (NHWC,
    :func:`nchw_to_nhwc`): x_nhwc [B, H, W, C], boxes [K, 4] xyxy, rand [K, n_mc, PH, PW] -> h [K, C] f64.  The
    (K, C, PH, PW) tensor of ``roi_align`` is never written; same bits as ``roi_align`` + :func:`mc_entropy`.  Calls of
    more than 65 535 ROIs are cut in slices."""
    require_gpu()
    assert x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    b, hh, ww, c = x_nhwc.shape
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    boxes = boxes.to(device=x_nhwc.device, dtype=torch.float32).contiguous()
    kk = boxes.shape[0]
    if batch_idx is not None:
        batch_idx = batch_idx.to(device=x_nhwc.device, dtype=torch.int32).contiguous()
    if isinstance(rand, CounterDraws):
        rand = _explicit_counter_draws(rand, kk, n_mc, ph, pw)  # (same bits as the in-kernel generator)
    if rand is not None:
        rand = rand.to(device=x_nhwc.device, dtype=torch.float32).contiguous()
        assert rand.shape == (kk, n_mc, ph, pw)
    h = torch.empty((kk, c), dtype=torch.float64, device=x_nhwc.device)
    z = torch.empty((kk * n_mc, c), dtype=torch.float32, device=x_nhwc.device) if return_samples else None
    for k0, n in _image_slices(kk):
        ws_bytes = query("runia_roi_mc_entropy_workspace_bytes", n, ph, pw, n_mc, sampling_ratio)
        ws = workspace(ws_bytes, x_nhwc.device)
        launch("runia_roi_mc_entropy_f32", x_nhwc.data_ptr(), boxes[k0:].data_ptr(),
               None if batch_idx is None else batch_idx[k0:].data_ptr(), None if rand is None else rand[k0:].data_ptr(),
               n_mc * ph * pw, h[k0:].data_ptr(), None if z is None else z[k0 * n_mc:].data_ptr(), ws.data_ptr(), ws_bytes, n, b,
               c, hh, ww, int(ph), int(pw), float(spatial_scale), int(sampling_ratio), 1 if aligned else 0, int(n_mc),
               float(drop_prob), int(block_size), int(k), float(min_dist))
    return (h, z) if return_samples else h


ROI_MEANS_MAX_HW = _HEADER_MACROS["RUNIA_ROI_MEANS_MAX_HW"]  # H + W of one feature map (the per-axis weights live in LDS)


def roi_means_supported(x_nhwc_shape) -> bool:
    """Whether :func:`roi_means` takes a map of this ``[B, H, W, C]`` shape (else: ``roi_align`` + ``mean``)."""
    _, hh, ww, c = x_nhwc_shape
    return hh + ww <= ROI_MEANS_MAX_HW and hh * ww * c * 4 < ROI_FUSED_MAX_IMAGE_BYTES


@_device_guard("boxes", "batch_idx", "out")
def roi_means(x_nhwc: torch.Tensor, boxes: torch.Tensor, output_size, spatial_scale: float, sampling_ratio: int,
              aligned: bool, batch_idx: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              col_offset: int = 0) -> torch.Tensor:
    """``roi_align(x, boxes, output_size, spatial_scale, sampling_ratio, aligned).mean((2, 3))`` in ONE pass from the
    feature map (NHWC, :func:`nchw_to_nhwc`): x_nhwc [B, H, W, C], boxes [K, 4] xyxy -> [K, C] f32.  The (K, C, PH, PW)
    tensor is never written.  ``out`` (additive): a ``(K, C_total)`` f32 device matrix with unit column stride whose columns
    ``col_offset : col_offset + C`` receive the means (one slice per hooked layer, no concatenation); it is returned."""
    require_gpu()
    assert x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
    b, hh, ww, c = x_nhwc.shape
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    boxes = boxes.to(device=x_nhwc.device, dtype=torch.float32).contiguous()
    kk = boxes.shape[0]
    if batch_idx is not None:
        batch_idx = batch_idx.to(device=x_nhwc.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty((kk, c), dtype=torch.float32, device=x_nhwc.device)
        col_offset = 0
    assert out.dtype == torch.float32 and out.device == x_nhwc.device and out.dim() == 2 and out.shape[0] == kk
    assert out.stride(1) == 1 and 0 <= col_offset and col_offset + c <= out.shape[1]
    launch("runia_roi_means_f32", x_nhwc.data_ptr(), boxes.data_ptr(), _ptr(batch_idx), out.data_ptr(),
           out.stride(0) if kk > 1 else out.shape[1], int(col_offset), kk, b, c, hh, ww, int(ph), int(pw), float(spatial_scale),
           int(sampling_ratio), 1 if aligned else 0)
    return out


KDE_KERNELS = ("gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine")


@_device_guard()
def kde_score_kernel(train: torch.Tensor, x: torch.Tensor, bandwidth: float, kernel: str) -> torch.Tensor:
    """log-density of ``x`` [N, D] under a kernel density estimate on ``train`` [M, D] (both f64) for any of sklearn's
    kernels (``KDE_KERNELS``) with sklearn's normalisation -> [N] f64."""
    require_gpu()
    assert kernel in KDE_KERNELS, f"unknown kernel {kernel!r}"
    assert train.is_cuda and x.is_cuda and train.dtype == torch.float64 and x.dtype == torch.float64
    train, x = train.contiguous(), x.contiguous()
    s = torch.empty((x.shape[0],), dtype=torch.float64, device=x.device)
    launch("runia_kde_score_kernel_f64", train.data_ptr(), x.data_ptr(), s.data_ptr(), train.shape[0], x.shape[0], train.shape[1],
           float(bandwidth), KDE_KERNELS.index(kernel))
    return s


@_device_guard()
def clock_probe(chain: int = 8192, device: Optional[torch.device] = None) -> torch.Tensor:
    """Queue one clock probe (``runia_clock_probe``) on the current stream -> device tensor [4] int64
    (shader-clock ticks, 100 MHz ticks, FMAs in the chain, 0).  Read it with :func:`clock_ghz` after a synchronisation."""
    dev = require_gpu() if device is None else torch.device(device)
    with torch.cuda.device(dev):  # the probe runs on `dev`'s stream and reads `dev`'s clock, whatever device is current
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        launch("runia_clock_probe", out.data_ptr(), int(chain))
    return out


def clock_ghz(probe: torch.Tensor) -> dict:
    """Host reading of a finished :func:`clock_probe`: the clock held (GHz), the probe's length and the cycles one
    dependent f32 FMA took."""
    t, r, n, _ = (int(v) for v in probe.cpu().tolist())
    ns = r * 10.0
    return {"ghz": round(t / ns, 4) if ns > 0 else None, "probe_us": round(ns / 1e3, 2),
            "cycles_per_dependent_fma": round(t / n, 3) if n else None}


@_device_guard()
def tril_inverse(tril: torch.Tensor) -> torch.Tensor:
    """tril [B, D, D] f64 lower-triangular (device) -> their inverses [B, D, D] (``runia_tril_inverse_f64``)."""
    require_gpu()
    assert tril.is_cuda and tril.dtype == torch.float64 and tril.dim() == 3 and tril.shape[1] == tril.shape[2]
    tril = tril.contiguous()
    out = torch.empty_like(tril)
    launch("runia_tril_inverse_f64", tril.data_ptr(), out.data_ptr(), tril.shape[0], tril.shape[1])
    return out


_GMM_WORKSPACE_CAP = 1 << 30  # bytes of per-tile sums kept at once (262 144 rows x 2048 x 10 classes: 336 MB)


@_device_guard()
def gmm_log_prob(x: torch.Tensor, means: torch.Tensor, w_tril: torch.Tensor, consts: torch.Tensor, want_log_prob: bool = True,
                 want_lse: bool = False):
    """Class-wise Gaussian log densities with the inverse Cholesky factors (``runia_gmm_log_prob_f32``): x [N, D] f32, means [C, D] f32,
    w_tril [C, D, D] f32 lower triangular (= L_c^-1), consts [C] f64 -> ``(log_prob [N, C] f32 or None, lse [N] f32 or None)``."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    assert means.dtype == torch.float32 and w_tril.dtype == torch.float32 and consts.dtype == torch.float64
    n, d = x.shape
    c = means.shape[0]
    assert tuple(means.shape) == (c, d) and tuple(w_tril.shape) == (c, d, d) and tuple(consts.shape) == (c,)
    assert want_log_prob or want_lse
    x, means, w_tril, consts = x.contiguous(), means.contiguous(), w_tril.contiguous(), consts.contiguous()
    lp = torch.empty((n, c), dtype=torch.float32, device=x.device) if want_log_prob else None
    lse = torch.empty((n,), dtype=torch.float32, device=x.device) if want_lse else None
    if n == 0:
        return lp, lse
    need = query("runia_gmm_log_prob_workspace_bytes", n, d, c)
    ws_bytes = min(need, max(_GMM_WORKSPACE_CAP, need // max(1, n) * 128))  # the entry point scores the rows in chunks that fit
    ws = workspace((ws_bytes + 7) // 8 * 8, x.device, 0)
    launch("runia_gmm_log_prob_f32", x.data_ptr(), means.data_ptr(), w_tril.data_ptr(), consts.data_ptr(), _ptr(lp), _ptr(lse),
           ws.data_ptr(), ws.numel(), n, d, c)
    return lp, lse


@_device_guard()
def kth_smallest_flat(x: torch.Tensor, ranks) -> list:
    """Exact order statistics of a float32 device tensor read as one flat array: ``sorted(x.flatten())[k]`` for every ``k`` of
    ``ranks`` (0-based), as Python floats holding float32 values.  Radix select: three histogram passes per rank
    (``runia_select_hist_f32``), one 8 KB read-back per pass.  Setup-time (synchronises).  The array must not contain NaNs (their
    keys sort above +inf; NumPy's partition puts them last as well, but its percentile then returns NaN: the caller checks)."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    n = x.numel()
    hist = torch.empty((2048,), dtype=torch.int32, device=x.device)
    out = []
    for k in ranks:
        k = int(k)
        assert 0 <= k < n
        prefix, mask = 0, 0
        for shift, width in ((21, 11), (10, 11), (0, 10)):
            launch("runia_select_hist_f32", x.data_ptr(), hist.data_ptr(), n, prefix, mask, shift)
            h = hist.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            cum = np.cumsum(h)
            b = int(np.searchsorted(cum, k, side="right"))
            assert b < 2048 and h[b] > 0, "radix select lost the rank (NaNs in the array?)"
            k -= int(cum[b - 1]) if b else 0
            prefix |= (b & ((1 << width) - 1)) << shift  # (the last pass's 11-bit digit repeats bit 10, already in the prefix)
            mask |= ((1 << width) - 1) << shift
        bits = (prefix & 0x7FFFFFFF) if (prefix & 0x80000000) else (~prefix & 0xFFFFFFFF)
        out.append(float(np.array([bits], dtype=np.uint32).view(np.float32)[0]))
    return out


@_device_guard()
def cholesky(a: torch.Tensor, jitter: float = 0.0):
    """a [B, D, D] (or [D, D]) f32 / f64 symmetric on the device -> ``(L, info)``: the lower Cholesky factors of ``a + jitter * I``
    (a new tensor; zeros above the diagonal) and ``info`` [B] int32 on the device - 0, or j + 1 where column j's pivot was not
    positive (``runia_cholesky_*``)."""
    require_gpu()
    assert a.is_cuda and a.dtype in (torch.float32, torch.float64) and a.dim() in (2, 3) and a.shape[-1] == a.shape[-2]
    m = a.reshape(-1, a.shape[-1], a.shape[-1]).contiguous().clone()
    info = torch.empty((m.shape[0],), dtype=torch.int32, device=a.device)
    launch("runia_cholesky_f32" if a.dtype == torch.float32 else "runia_cholesky_f64", m.data_ptr(), info.data_ptr(), m.shape[0],
           m.shape[1], float(jitter))
    return m.reshape(a.shape), info


NMS_SORT_MAX = _HEADER_MACROS["RUNIA_NMS_SORT_MAX"]  # keys one workgroup sorts in LDS (longer lists: torch.sort of the same keys)
NMS_MAX_BOXES = _HEADER_MACROS["RUNIA_NMS_MAX_BOXES"]  # boxes one greedy walk takes (its removed bitmap lives in LDS)
YOLO_MAX_ANCHORS = _HEADER_MACROS["RUNIA_YOLO_MAX_ANCHORS"]


def nms_workspace_bytes(m: int) -> int:
    """Bytes of the IoU bitmask of ``m`` sorted boxes: ``m * ceil(m / 64) * 8``."""
    return query("runia_nms_workspace_bytes", int(m))


@_device_guard()
def nms_sorted_keys(scores: torch.Tensor) -> torch.Tensor:
    """scores [n] f32 (device) -> the int64 keys ``(desc(score) << 31) | i`` in ascending order = descending score, ties by
    ascending index, every NaN (desc = 0) in front of +inf (``runia_nms_keys_f32``, then ``runia_nms_sort_keys`` up to :data:`NMS_SORT_MAX` keys, a device
    ``torch.sort`` of the same distinct keys above: one order either way)."""
    require_gpu()
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 1
    n = scores.shape[0]
    assert n <= 0x7FFFFFFF
    keys = torch.empty((n,), dtype=torch.int64, device=scores.device)
    if n == 0:
        return keys
    scores = scores.contiguous()
    launch("runia_nms_keys_f32", scores.data_ptr(), n, keys.data_ptr())
    if n <= NMS_SORT_MAX:
        launch("runia_nms_sort_keys", keys.data_ptr(), n)
        return keys
    return torch.sort(keys, stable=True).values


@_device_guard()
def nms_sorted(boxes: torch.Tensor, sorted_keys: torch.Tensor, iou_threshold: float, max_det: Optional[int] = None):
    """Greedy NMS of the boxes [*, 4] xyxy f32 (device) in the order of ``sorted_keys`` (:func:`nms_sorted_keys`, possibly
    truncated) -> ``(keep, count)``: int64 device tensors, ``keep[:count]`` the kept boxes' indices (at most ``max_det``),
    in sorted order (``runia_nms_sorted_f32``).  Nothing is read back here."""
    require_gpu()
    assert boxes.is_cuda and boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == 4
    assert sorted_keys.dtype == torch.int64 and sorted_keys.dim() == 1 and sorted_keys.device == boxes.device
    m = sorted_keys.shape[0]
    if m > NMS_MAX_BOXES:
        raise RuniaHipError(f"nms: {m} boxes, at most {NMS_MAX_BOXES} per call")
    max_det = m if max_det is None else max(0, min(int(max_det), m))
    boxes, sorted_keys = boxes.contiguous(), sorted_keys.contiguous()
    keep = torch.empty((max(max_det, 1),), dtype=torch.int64, device=boxes.device)
    count = torch.zeros((1,), dtype=torch.int64, device=boxes.device)
    ws_bytes = nms_workspace_bytes(m)
    ws = workspace(ws_bytes, boxes.device, 0) if ws_bytes else None
    launch("runia_nms_sorted_f32", boxes.data_ptr(), sorted_keys.data_ptr(), m, float(iou_threshold), max_det, keep.data_ptr(),
           count.data_ptr(), _ptr(ws), ws_bytes)
    return keep, count


@_device_guard("classes")
def yolo_candidates(pred: torch.Tensor, nc: int, conf_thres: float, classes=None, max_wh: float = 0.0):
    """One image's YOLOv8 head ``pred`` [4 + nc + nm, A] f32 (device, channel-major) -> its candidates in anchor order
    (``runia_yolo_candidates_f32``): ``(boxes [A, 4] = rows 0-3 + best class * max_wh, scores [A], anchor [A] int32,
    cls [A] int32, count)`` with ``count`` an int64 device tensor [1]; the first ``count`` rows are valid."""
    require_gpu()
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2
    c, a = pred.shape
    nm = c - 4 - int(nc)
    assert nc >= 1 and nm >= 0, "head rows must be 4 + nc + nm"
    if a > YOLO_MAX_ANCHORS:
        raise RuniaHipError(f"yolo_candidates: {a} anchors, at most {YOLO_MAX_ANCHORS}")
    dev = pred.device
    pred = pred.contiguous()
    cls_list = None
    if classes is not None:
        cls_list = torch.as_tensor(classes).reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    boxes = torch.empty((a, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((a,), dtype=torch.float32, device=dev)
    anchor = torch.empty((a,), dtype=torch.int32, device=dev)
    cls = torch.empty((a,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    if a == 0:
        return boxes, scores, anchor, cls, count
    ws_bytes = query("runia_yolo_candidates_workspace_bytes", a)
    ws = workspace(ws_bytes, dev, 0)
    n_cls = 0 if cls_list is None else int(cls_list.numel())
    launch("runia_yolo_candidates_f32", pred.data_ptr(), a, int(nc), nm, float(conf_thres), _ptr(cls_list) if n_cls else None,
           n_cls, float(max_wh), boxes.data_ptr(), scores.data_ptr(), anchor.data_ptr(), cls.data_ptr(), count.data_ptr(),
           ws.data_ptr(), ws_bytes)
    return boxes, scores, anchor, cls, count


PACMAP_MAX_K = _HEADER_MACROS["RUNIA_PACMAP_MAX_K"]  # neighbour candidates per row of the kNN graph
PACMAP_MAX_MN = _HEADER_MACROS["RUNIA_PACMAP_MAX_MN"]
PACMAP_MAX_FP = _HEADER_MACROS["RUNIA_PACMAP_MAX_FP"]
PACMAP_MAX_COMPONENTS = _HEADER_MACROS["RUNIA_PACMAP_MAX_COMPONENTS"]
PACMAP_KIND_NB, PACMAP_KIND_MN, PACMAP_KIND_FP = (_HEADER_MACROS["RUNIA_PACMAP_KIND_" + k] for k in ("NB", "MN", "FP"))  # bits 30-31 of a grouped pair entry


@_device_guard()
def pacmap_knn(q: torch.Tensor, bank: torch.Tensor, k: int, exclude_self: bool):
    """Exact kNN of the rows of ``q`` [Q, D] among ``bank`` [N, D] (f32, device) -> ``(idx [Q, k] int32, dist [Q, k] f32)``,
    sorted by (distance, index); ``exclude_self`` leaves bank row i out of query row i's list (``runia_pacmap_knn_f32``)."""
    require_gpu()
    assert q.is_cuda and bank.is_cuda and q.dtype == torch.float32 and bank.dtype == torch.float32
    assert q.dim() == 2 and bank.dim() == 2 and q.shape[1] == bank.shape[1]
    q, bank = q.contiguous(), bank.contiguous()
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=q.device)
    dist = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    launch("runia_pacmap_knn_f32", q.data_ptr(), q.shape[0], bank.data_ptr(), bank.shape[0], bank.shape[1], int(k),
           int(bool(exclude_self)), idx.data_ptr(), dist.data_ptr())
    return idx, dist


@_device_guard()
def pacmap_pairs(x: torch.Tensor, bank: torch.Tensor, knn_idx: torch.Tensor, knn_dist: torch.Tensor, n_nb: int, n_mn: int,
                 n_fp: int, seed: int, transform: bool):
    """NB / MN / FP pair lists ``(pair_nb [R * n_nb, 2], pair_mn [R * n_mn, 2], pair_fp [R * n_fp, 2])`` int32 (device) of the
    rows ``x`` [R, D] against ``bank`` [Nb, D] from their kNN table (``runia_pacmap_pairs``; the fit passes ``x is bank``)."""
    require_gpu()
    assert x.dtype == torch.float32 and bank.dtype == torch.float32 and knn_idx.dtype == torch.int32
    assert knn_dist.dtype == torch.float32 and knn_idx.shape == knn_dist.shape and knn_idx.shape[0] == x.shape[0]
    x, bank, knn_idx, knn_dist = x.contiguous(), bank.contiguous(), knn_idx.contiguous(), knn_dist.contiguous()
    r, d = x.shape
    dev = x.device
    nb = torch.empty((r * n_nb, 2), dtype=torch.int32, device=dev)
    mn = torch.empty((r * n_mn, 2), dtype=torch.int32, device=dev)
    fp = torch.empty((r * n_fp, 2), dtype=torch.int32, device=dev)
    ws_bytes = 0 if transform else query("runia_pacmap_pairs_workspace_bytes", r)
    ws = workspace(ws_bytes, dev, 0) if ws_bytes else None
    launch("runia_pacmap_pairs", x.data_ptr(), r, bank.data_ptr(), bank.shape[0], d, knn_idx.data_ptr(), knn_dist.data_ptr(),
           knn_idx.shape[1], int(n_nb), int(n_mn), int(n_fp), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(transform)), nb.data_ptr(),
           mn.data_ptr() if n_mn else None, fp.data_ptr() if n_fp else None, _ptr(ws), ws_bytes)
    return nb, mn, fp


def pacmap_phase_weights(t: int):
    """``(w_NB, w_MN, w_FP)`` of iteration ``t`` as the step kernel uses them (``runia_pacmap_phase_weights``, host only)."""
    w = (c_float * 3)()
    call("runia_pacmap_phase_weights", int(t), ctypes.addressof(w))
    return tuple(float(v) for v in w)


@_device_guard()
def pacmap_step(y_in: torch.Tensor, y_part: torch.Tensor, y_out: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                offsets: torch.Tensor, entries: torch.Tensor, t: int, lr: float) -> torch.Tensor:
    """One Adam iteration ``t`` of the rows ``y_in`` [R, C] into ``y_out`` (``runia_pacmap_step_f32``); ``m`` / ``v`` are
    updated in place.  Row r's pairs: ``entries[offsets[r]:offsets[r + 1]]`` = ``(kind << 30) | partner``, partners read
    from ``y_part``.  All operands contiguous f32 / int64 / int32 on one device."""
    require_gpu()
    r, c = y_in.shape
    for a, dt in ((y_in, torch.float32), (y_part, torch.float32), (y_out, torch.float32), (m, torch.float32),
                  (v, torch.float32), (offsets, torch.int64), (entries, torch.int32)):
        assert a.is_cuda and a.dtype == dt and a.is_contiguous()
    assert y_out.shape == y_in.shape == m.shape == v.shape and y_part.shape[1] == c and offsets.shape[0] == r + 1
    launch("runia_pacmap_step_f32", y_in.data_ptr(), y_part.data_ptr(), y_out.data_ptr(), m.data_ptr(), v.data_ptr(),
           offsets.data_ptr(), entries.data_ptr(), r, c, int(t), float(lr))
    return y_out
