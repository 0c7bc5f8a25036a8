"""torch.autograd wrappers over the C ABI (include/mvkpconv.h).

PyTorch only owns the HBM buffers and the HIP stream; all compute below is in libmvkpconv.so.
Every function requires CUDA(HIP) tensors and raises otherwise -- there is no CPU path here.
"""
import collections
import os
import ctypes as C

import weakref

import torch

from ._lib import lib, check, CONSTANTS, SCENE_CONSTANTS, TRAIN_CONSTANTS, SPHERE_CONSTANTS

# the MVK_INFL_* / MVK_AGG_* codes of include/mvkpconv.h under the reference's names (blocks.py:329-354)
INFLUENCE = {k[len("MVK_INFL_"):].lower(): v for k, v in CONSTANTS.items() if k.startswith("MVK_INFL_")}
AGGREGATION = {k[len("MVK_AGG_"):].lower(): v for k, v in CONSTANTS.items() if k.startswith("MVK_AGG_")}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("MV-KPConv ops need tensors resident in HBM (got a CPU tensor); "
                               "there is no CPU fallback")


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _idx(t):
    if t.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("neighbour indices must be int32 or int64")
    return t.contiguous(), int(t.dtype == torch.int64)


# --------------------------------------------------------------------------------------------
# zero arena (opt-in): one fill per step instead of one per zero-initialised output
# --------------------------------------------------------------------------------------------
# Split-K GEMM outputs and scatter targets must start at zero; eagerly that is ~100 tiny fill kernels per
# step. With the arena enabled, step_begin() zeroes one big buffer with a single launch and _zeros()
# hands out 256-byte aligned slices of it. Slices are only valid until the next step_begin(): this is for
# the captured-graph step of bench.py (fixed addresses), not a general allocator.
_ARENA = {"on": False, "buf": None, "off": 0, "high": 0}


def zero_arena_enable(nbytes, device):
    _ARENA.update(on=True, buf=torch.zeros(int(nbytes), dtype=torch.uint8, device=device), off=0)


def zero_arena_disable():
    _ARENA.update(on=False, buf=None, off=0)


def zero_arena_high_water(reset=False):
    """Largest number of bytes _zeros() handed out (or would have) between two step_begin() calls;
    reset=True starts a new measurement (call it right before the steps that size the arena)."""
    if reset:
        _ARENA["off"] = 0
        _ARENA["high"] = 0
    return _ARENA["high"]


def step_begin():
    _ARENA["high"] = max(_ARENA["high"], _ARENA["off"])
    _ARENA["off"] = 0
    if _ARENA["on"]:
        _ARENA["buf"].zero_()


def _zeros(shape, device, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= int(s)
    nbytes = (n * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
    off = _ARENA["off"]
    _ARENA["off"] = off + nbytes
    if _ARENA.get("log") is not None:
        import traceback
        _ARENA["log"].append((nbytes, tuple(shape), traceback.extract_stack(limit=3)[0].name))
    buf = _ARENA["buf"]
    if _ARENA["on"] and n > 0 and off + nbytes <= buf.numel() and buf.device == device:
        return buf[off:off + nbytes].view(dtype)[:n].view(shape)
    return torch.zeros(shape, device=device, dtype=dtype)


# --------------------------------------------------------------------------------------------
# raw kernels
# --------------------------------------------------------------------------------------------

# --------------------------------------------------------------------------------------------
# deterministic mode: ordered reductions (run-to-run bit-identical products, no zero-initialised outputs)
# --------------------------------------------------------------------------------------------
# By default a product whose reduction is split over workgroups adds its partial sums with f32 atomics: the fastest way
# (fire and forget), but the sum depends on the order the workgroups ran in -- rounding only, yet a LeakyReLU input within
# an ulp of zero then takes the other slope and two runs of one network differ visibly. set_deterministic(True) (or
# MVK_DETERMINISTIC=1) hands the library an arena (mvk_gemm_split_arena): every split product then parks its partial
# tiles in HBM and the last-arriving workgroup of a tile adds them in split order (csrc/gemm.hip), the bias gradient of
# the BatchNorm-less layers is summed in workgroup order, outputs need no zero fill and split plans keep their
# BatchNorm-statistics epilogue. The price is three memory-side round trips at the tail of every split launch (~4 us
# each, +0.2 ms on the 4.1 ms early-fusion step): opt-in, like torch.use_deterministic_algorithms.
_DET = {"on": os.environ.get("MVK_DETERMINISTIC", "0") == "1"}
_SPLIT_ARENA = {}
_SPLIT_ARENA_BYTES = int(os.environ.get("MVK_GEMM_ARENA_MB", "1024")) << 20
_SPLIT_COUNTERS = 1 << 20


def set_deterministic(flag, device=None):
    """Turns the ordered reductions on or off (see above). Turning them on creates the arena on `device` (default: the
    current one) at once: do it outside any graph capture."""
    _DET["on"] = bool(flag)
    # (torch.backends.cudnn.deterministic is NOT touched: on this image it drops MIOpen to naive convolution kernels, 4 ms
    # -> 226 ms per step; the frozen 2D encoder is a library network outside this mode)
    if flag:
        split_arena_prepare(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    else:
        split_arena_release()


def is_deterministic():
    """True when the ordered reductions are on. With MVK_DETERMINISTIC=1 the arena used to appear only with the first
    product, so a pyramid built before it saw False (rows in arrival order, no transposed upsampling lists: the first
    step of an env-enabled run was not bit-reproducible): the first question creates the arena."""
    if _DET["on"] and not _SPLIT_ARENA and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        split_arena_prepare(torch.device("cuda", torch.cuda.current_device()))
    return bool(_DET["on"] and _SPLIT_ARENA)


def split_arena_prepare(device):
    """Creates the arena of the ordered reductions on `device` in deterministic mode (no-op otherwise, or when it exists).
    Called by the first product; call it (or set_deterministic) yourself before capturing a graph that was never run
    eagerly."""
    if not _DET["on"]:
        return False
    device = torch.device(device)
    if device.index in _SPLIT_ARENA:
        return True
    if _SPLIT_ARENA:
        raise RuntimeError("the ordered reductions use ONE arena per process (one GPU per process); it lives on "
                           "cuda:%d" % next(iter(_SPLIT_ARENA)))
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("ops: the arena of the ordered reductions does not exist yet and cannot be created inside a "
                           "graph capture; run one eager step first or call ops.set_deterministic(True) before")
    ws = torch.empty(_SPLIT_ARENA_BYTES, dtype=torch.uint8, device=device)
    cnt = torch.zeros(_SPLIT_COUNTERS, dtype=torch.int32, device=device)
    torch.cuda.current_stream(device).synchronize()          # the counters are zero before any stream uses them
    check(lib().mvk_gemm_split_arena(_p(ws), ws.numel(), _p(cnt), cnt.numel()))
    _SPLIT_ARENA[device.index] = (ws, cnt)
    return True


def split_arena_release():
    """Back to the atomic split reductions; frees the arena."""
    if _SPLIT_ARENA:
        torch.cuda.synchronize()
        check(lib().mvk_gemm_split_arena(None, 0, None, 0))
        _SPLIT_ARENA.clear()


def _split_out(shape, device, split, keep=False):
    """Output buffer of a product whose reduction is split `split` ways: the ordered reduction writes every element
    (empty); the atomic one accumulates onto zeros (arena slice, or a tensor of its own when it outlives the step)."""
    if split <= 1 or device.index in _SPLIT_ARENA:
        return torch.empty(shape, device=device, dtype=torch.float32)
    return torch.zeros(shape, device=device, dtype=torch.float32) if keep else _zeros(shape, device)


def gemm_plan(M, N, Kd, split_k=None, want_stats=False):
    """(split, stat_rows) mvk_gemm_f32_ex will use for this shape: the split of the reduction (the output must
    be zero-initialised when > 1) and the row-block size of the BatchNorm partials (0 = none produced)."""
    sp, rows = C.c_int(0), C.c_int(0)
    check(lib().mvk_gemm_f32_plan(int(M), int(N), int(Kd), int(split_k or 0), int(bool(want_stats)), C.byref(sp),
                                  C.byref(rows)))
    return sp.value, rows.value


def kpconv_gather_plan(Nq, Ns, H, Cin, elem_bytes=4, deformable=False):
    """Launch geometry of the MFMA gather for a (linear, sum) layer (mvk_kpconv_gather_plan): 'mfma' 1,
    'lanes_per_point' 64, 'points_per_wave' 1, 'rows_per_batch' (its channel tiles per wave), 'first_sharing_workgroup'
    (0: the four waves of a workgroup share one point, -1: one point each), 'waves_per_workgroup' 4, 'workgroups' and
    'grid_threads'. Every value is 0 when the layer runs on the lane = channel kernel, one point per wave."""
    out = (C.c_int64 * 8)()
    check(lib().mvk_kpconv_gather_plan(int(Nq), int(Ns), int(H), int(Cin), int(elem_bytes), int(bool(deformable)), out))
    keys = ("lanes_per_point", "points_per_wave", "rows_per_batch", "first_sharing_workgroup", "waves_per_workgroup",
            "workgroups", "grid_threads", "mfma")
    return dict(zip(keys, [int(v) for v in out]))


# rows up to which a BatchNorm takes its statistics from the producing GEMM's epilogue: every workgroup of the
# normalising launch merges ALL the epilogue's (sum, M2) partials of its channels, one per 64 rows -- beyond a few
# hundred of them (FeatureAggregation's 58 392 rows: 913) the separate statistics launch is the cheaper way
_STATS_EPILOGUE_ROWS = int(os.environ.get("MVK_GEMM_STATS_MAX_ROWS", "32768"))

BN_SMALL_ROWS = 128      # csrc/bn.hip: up to this many rows one launch does statistics and normalisation (any D)


def bn_single_launch_rows(D):
    """Rows up to which the BatchNorm of a D-channel input is one launch (csrc/bn.hip: 128, or 1024 when D % 4 == 0):
    the producing GEMM then skips its statistics epilogue."""
    return lib().mvk_bn_single_launch_rows(int(D))


# --------------------------------------------------------------------------------------------
# BatchNorm folded into the products around it (round 5; csrc/gemm.hip GemmArgs (a), (b))
# --------------------------------------------------------------------------------------------
# The producer's half: a product that writes the statistics partials of its output can also FINISH them (mean, invstd,
# running statistics, batch counter) -- the workgroup that arrives last at a column tile's counter merges the partials.
# The consumer's half: bn_lrelu_linear(), the BatchNorm's apply pass inside the next product's operand load.
# The hand-off from a product to the BatchNorm behind it is ONE record, BnStats, and it travels by argument and return value:
#   created where the launch that wrote the partials is issued: _product() (linear, upsample_cat_linear, kpconv),
#     _LinearPairFn (one record per output) and _KPConvFn around gemm_f32_stream (the big rigid layers; never finished).
#     The op wrappers take `bn=` (the nn.BatchNorm1d that follows); when _finishable(bn) they hand it to their autograd
#     node as a plain forward argument, the node hands it to the product, and the record comes back as a non-tensor
#     output of the node;
#   attached by the op wrapper to its output as `_mvk_bn_stats` (tests attach a plain (partials, rows) tuple by hand);
#   read by bn_stats_of() alone, which normalises what it finds: bn_lrelu / bn_lrelu_pair (_bn_fwd_problem), bn_finished,
#     bn_lrelu_linear.
# MEASURED SLOWER on the one-sphere step and therefore OFF by default (MVK_BN_FOLD=1 / ops.BN_FOLD = True turn it on):
# network chain 2.85 -> 2.94 ms with finished statistics alone, 2.96 ms with the operand fold on top (round 5,
# profiles/r05_bn_fold_chain.txt). The last-arriver hand-off at the tail of a producing product costs
# +5..13 us per launch (store acknowledge, counter round trip, 3-5 dependent rounds of memory-side loads over up to 305
# partials) against the 2-4 us the normalising launch saves by not reducing them, and in a bottleneck block with a
# shortcut layer the convolution's BatchNorm already shares its launch with the shortcut's.
BN_FOLD = os.environ.get("MVK_BN_FOLD", "0") == "1"
# partials [row blocks, 2, N], rows per block, finished = (mean, invstd) written by the producing launch or None
BnStats = collections.namedtuple("BnStats", "partials rows finished", defaults=(None,))


def bn_stats_of(t):
    """The BnStats a producing product attached to its output t for the BatchNorm that follows, or None. A plain
    (partials, rows[, finished]) tuple found there (attached by hand) is normalised."""
    e = getattr(t, "_mvk_bn_stats", None)
    return e if e is None or isinstance(e, BnStats) else BnStats(*e)


def bn_finished(t):
    """True when t carries BatchNorm statistics FINISHED by its producer (mean, invstd)."""
    return getattr(bn_stats_of(t), "finished", None) is not None


def _finishable(bn):
    """Whether a product may finish the statistics of the BatchNorm that follows it: only training-mode modules with
    per-rank statistics qualify; anything else keeps the separate statistics pass."""
    return BN_FOLD and bn is not None and bn.training and _SYNC_BN["group"] is None and bn.num_features % 4 == 0


def _fin_counters(bn, device):
    """Persistent zero int32 words of one BatchNorm module (the kernel returns them to zero): one per column tile."""
    c = getattr(bn, "_mvk_fin_counters", None)
    if c is None or c.device != device:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ops: the finish counters of a BatchNorm do not exist yet and cannot be created inside a "
                               "graph capture; run one eager step first")
        c = torch.zeros(128, dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()
        bn._mvk_fin_counters = c
    return c


def _fin_struct(bn, N, device):
    from ._lib import BnFinish
    if bn.num_features != N:
        raise RuntimeError("ops: the BatchNorm handed to a product has %d channels, the product %d columns" % (bn.num_features, N))
    mean = torch.empty(N, device=device, dtype=torch.float32)
    invstd = torch.empty(N, device=device, dtype=torch.float32)
    track = bn.track_running_stats and bn.running_mean is not None
    fin = BnFinish(_p(_fin_counters(bn, device)), float(bn.eps), float(bn.momentum if bn.momentum is not None else 0.0),
                   _p(mean), _p(invstd), _p(bn.running_mean) if track else None, _p(bn.running_var) if track else None,
                   _p(bn.num_batches_tracked) if track else None)
    return fin, (mean, invstd)


def gemm(A, B, transA=False, transB=False, out=None, accumulate=False, split_k=None, keep=False, stats_n_valid=None):
    """C = op(A) @ op(B) on v_mfma_f32_16x16x4_f32 (mvk_gemm_f32_ex). split_k=None lets the library pick the
    row tile and the split of the reduction so that small-M / deep-K products (the coarse KPConv layers:
    85 x 7680 x 512) still fill the 256 CUs. keep=True: the result outlives the step (a weight gradient that
    becomes .grad), so it must not be a slice of the per-step zero arena. out: the caller's [M,N] buffer; without
    `accumulate` it ends up holding the product alone whatever it held before (a split reduction that adds with atomics
    gets it zero-filled first).
    stats_n_valid (DEVICE int32 [1]): also produce the column statistics of C over its first n_valid rows for
    the BatchNorm that follows; returns (C, (partials, rows per block)) -- or (C, None) when the chosen plan
    splits the reduction."""
    out, st = _product(A, B, transA=transA, transB=transB, out=out, accumulate=accumulate, split_k=split_k, keep=keep,
                       stats_n_valid=stats_n_valid)
    if stats_n_valid is None:
        return out
    return out, (st[:2] if st is not None else None)


def _product(A, B, *, transA=False, transB=False, out=None, accumulate=False, split_k=None, keep=False,
             stats_n_valid=None, finish=None, a_transform=None):
    """gemm() for the autograd nodes: returns (C, BnStats or None). finish: the nn.BatchNorm1d that follows (the caller
    asked _finishable); it is finished inside the launch when the product carries the statistics epilogue, is not
    transposed on the A side and picks its own split. a_transform (bn_lrelu_linear): the BatchNorm + LeakyReLU applied
    to A while it is staged; A must be the transform's lazy tensor, which the launch writes on the way."""
    _dev(A, B)
    A, B = _f32c(A), _f32c(B)
    M, Kd = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    N = B.shape[0] if transB else B.shape[1]
    assert (B.shape[1] if transB else B.shape[0]) == Kd, "gemm: inner dimensions differ"
    ax = a_transform
    if ax is not None and (ax["lazy"].data_ptr() != A.data_ptr() or transA or not transB or out is not None or accumulate
                           or M == 0):
        raise RuntimeError("ops: a product with an operand transform takes the lazy tensor as A, W as transposed B and "
                           "an output of its own")
    if M == 0 or N == 0 or Kd == 0:
        return (out.zero_() if out is not None else torch.zeros((M, N), device=A.device, dtype=torch.float32)), None
    split_arena_prepare(A.device)
    # a finished BatchNorm needs the epilogue statistics whatever the row count (the one-launch BatchNorm kernels of few
    # rows would otherwise do statistics + normalisation themselves: with a fold there is no such launch)
    stats_ok = stats_n_valid is not None and out is None and not accumulate and M <= _STATS_EPILOGUE_ROWS
    if finish is None and ax is None:
        stats_ok = stats_ok and M > bn_single_launch_rows(N)
    split, rows = gemm_plan(M, N, Kd, split_k, stats_ok)
    if out is None:
        out = _split_out((M, N), A.device, split, keep)
    elif split > 1 and not accumulate and A.device.index not in _SPLIT_ARENA:
        out.zero_()          # the atomic split adds onto the output: a caller's buffer starts from zero like our own
    part =torch.empty(((M + rows - 1) // rows, 2, N), device=A.device, dtype=torch.float32) if rows > 0 else None
    fin = done = None
    if finish is not None and part is not None and not transA and split_k is None:
        fin, done = _fin_struct(finish, N, A.device)
    if fin is not None or ax is not None:
        xf = None
        if ax is not None:
            from ._lib import ATransform
            xf = ATransform(_p(ax["mean"]), _p(ax["invstd"]), _p(ax["gamma"]), _p(ax["beta"]), float(ax["slope"]),
                            _p(ax["n_valid"]), _p(ax["lazy"]))
            A = ax["raw"]
        check(lib().mvk_gemm_f32_bn(_p(A), _p(B), _p(out), M, N, Kd, int(transB), _p(part),
                                    _p(stats_n_valid) if part is not None else None,
                                    C.byref(fin) if fin is not None else None, C.byref(xf) if xf is not None else None,
                                    _stream()))
    else:
        check(lib().mvk_gemm_f32_ex(_p(A), _p(B), _p(out), M, N, Kd, int(transA), int(transB), int(accumulate),
                                    int(split), _p(part), _p(stats_n_valid) if part is not None else None, _stream()))
    return out, (BnStats(part, rows, done) if part is not None else None)


def gemm_f32_stream_plan(M, N, Kd):
    """(runs on the streaming kernel, 16-row tiles per workgroup, workgroups, floats needed behind A) for
    C [M,N] = A [M,Kd] . B [Kd,N] in f32 (mvk_gemm_f32_stream_plan)."""
    out = (C.c_int64 * 4)()
    check(lib().mvk_gemm_f32_stream_plan(int(M), int(N), int(Kd), out))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3])


def _slack_floats(t):
    """Readable float32 elements behind the last element of the (contiguous) tensor t inside its own storage."""
    return t.untyped_storage().nbytes() // 4 - t.storage_offset() - t.numel()


def gemm_f32_stream(A, B, stats_n_valid=None):
    """C [M,N] f32 = A [M,Kd] . B [Kd,N] on the streaming f32 MFMA kernel (weights stationary in registers, rows of A as
    fragment loads). Returns (C, (partials, rows per block) or None). The caller checks gemm_f32_stream_plan and that A
    has the slack the plan asks for (kpconv_gather allocates it)."""
    _dev(A, B, stats_n_valid)
    A, B = _f32c(A), _f32c(B)
    M, Kd = A.shape
    N = B.shape[1]
    ok, tiles, wgs, need = gemm_f32_stream_plan(M, N, Kd)
    if not ok or B.shape[0] != Kd:
        raise RuntimeError("gemm_f32_stream: unsupported shape %d x %d x %d" % (M, N, Kd))
    y = torch.empty((M, N), device=A.device, dtype=torch.float32)
    part = torch.empty((wgs, 2, N), device=A.device, dtype=torch.float32) if stats_n_valid is not None else None
    check(lib().mvk_gemm_f32_stream(_p(A), _slack_floats(A), _p(B), _p(y), M, N, Kd, _p(stats_n_valid), _p(part), _stream()))
    return y, ((part, 16 * tiles) if part is not None else None)


# ---- optional per-launch timing of the gather kernel (bench.py roofline): HIP events on the
# current stream around the C-ABI call; nothing is recorded unless profile_reset(enabled=True).
_PROF = {"on": False, "rec": [], "gemm": []}


def profile_reset(enabled):
    _PROF["on"] = bool(enabled)
    _PROF["rec"] = []
    _PROF["gemm"] = []
    _PROF["h_eff"] = {}


def _timing_events():
    """Start / stop events for one launch. Eager steps are host-bound, so the queue is usually empty when
    the start event is enqueued and the event would also time the host's launch latency of the kernel
    behind it: a short device-side spin first keeps the GPU busy until start event, kernel and stop event
    are all queued."""
    torch.cuda._sleep(200000)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0, e1


def profile_collect_contraction():
    """{(M, Kd, N): {launches, total_ms, flops_per_launch}} of the forward K x Cin x Cout contraction
    (gemm_f32_mfma NN); flops = 2*M*Kd*N (SURVEY.md 8d F_mfma)."""
    torch.cuda.synchronize()
    out = {}
    for key, e0, e1 in _PROF["gemm"]:
        r = out.setdefault(key, {"launches": 0, "total_ms": 0.0, "flops_per_launch": 2.0 * key[0] * key[1] * key[2]})
        r["launches"] += 1
        r["total_ms"] += e0.elapsed_time(e1)
    return out


def _gather_kernel_label(Nq, Ns, H, Cin, deform, fast=True):
    """Name of the kernel mvk_kpconv_gather_fwd launches (fast: linear influence and sum aggregation)."""
    p = kpconv_gather_plan(Nq, Ns, H, Cin, 4, deform)
    if fast and p["mfma"]:
        return "kpconv_gather_mfma<T=%d>(1 point per wave)" % p["rows_per_batch"]
    return "kpconv_lane_channel<fwd,deform>" if deform else "kpconv_lane_channel<fwd>"


def profile_collect(h_eff=None):
    """{(kernel, Nq, Ns, H, Cin, K): {launches, total_ms, bytes_per_launch, ...}}; h_eff maps
    (Nq, Ns, H) -> mean number of real (non-shadow) neighbours per row."""
    torch.cuda.synchronize()
    out = {}
    for key, e0, e1 in _PROF["rec"]:
        r = out.setdefault(key, {"launches": 0, "total_ms": 0.0, "each_ms": []})
        r["launches"] += 1
        t = e0.elapsed_time(e1)
        r["total_ms"] += t
        r["each_ms"].append(t)
    for key, r in out.items():
        name, Nq, Ns, H, Cin, K = key
        he = _PROF.get("h_eff", {}).get((Nq, Ns, H)) if name.endswith("[dx]") else None
        if he is None:
            he = (h_eff or {}).get((Nq, Ns, H), H)
        # algorithmic bytes: feature row + xyz + int32 index per real neighbour,
        # query xyz, and the [Nq,K,Cin] aggregate written by the gather kernel
        sx = 4
        r["bytes_per_launch"] = Nq * he * (Cin * sx + 12 + 4) + Nq * 12 + Nq * K * Cin * sx
        r["kernel"] = name
        r["shape"] = {"Nq": Nq, "Ns": Ns, "H": H, "H_eff": he, "Cin": Cin, "K": K}
    return out


def kpconv_gather(q, s, idx, x, kp, extent, influence="linear", aggregation="sum", offsets=None,
                  want_min_d2=False, order=None, tag=None):
    """A[n,k,c] = sum_h w[n,h,k] x+[idx[n,h],c]; returns (A, min_d2 or None). order [Nq] int32 (a permutation of the
    query rows, e.g. sorted by grid cell): the order the points are WORKED on; the result does not depend on it."""
    _dev(q, s, idx, x, kp, offsets, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (q.shape[0],) or not order.is_contiguous()):
        raise RuntimeError("kpconv_gather: order must be a contiguous int32 tensor of Nq entries")
    q, s, x, kp = _f32c(q), _f32c(s), _f32c(x), _f32c(kp)
    idx, i64 = _idx(idx)
    Nq, Ns, H, Cin, K = q.shape[0], s.shape[0], idx.shape[1] if idx.dim() == 2 else 0, x.shape[1], kp.shape[0]
    if x.shape[0] != Ns:
        raise RuntimeError("kpconv: features and support points differ in length")
    # 64 floats of slack behind the aggregate: the streaming contraction reads up to 31 floats past the last row
    A = torch.empty(Nq * K * Cin + 64, device=q.device, dtype=torch.float32)[:Nq * K * Cin].view(Nq, K, Cin)
    min_d2 = min_arg = None
    if offsets is not None:
        offsets = _f32c(offsets)
        if want_min_d2:
            min_d2 = torch.empty((Nq, K), device=q.device, dtype=torch.float32)
            min_arg = torch.empty((Nq, K), device=q.device, dtype=torch.int32)
    if _PROF["on"]:
        e0, e1 = _timing_events()
    check(lib().mvk_kpconv_gather_fwd_ordered(_p(q), Nq, _p(s), Ns, _p(idx), i64, H, _p(x), Cin, _p(kp), K,
                                              float(extent), INFLUENCE[influence], AGGREGATION[aggregation],
                                              _p(offsets), _p(min_d2), _p(min_arg), _p(A), _p(order), _stream()))
    if _PROF["on"]:
        e1.record()
        name = _gather_kernel_label(Nq, Ns, H, Cin, offsets is not None, (influence, aggregation) == ("linear", "sum"))
        if tag:         # the gather-form feature gradient: its own class, with the mean length of ITS (reverse) rows
            name += tag
            _PROF.setdefault("h_eff", {})[(Nq, Ns, H)] = float((idx < Ns).sum().item()) / max(Nq, 1)
        _PROF["rec"].append(((name, Nq, Ns, H, Cin, K), e0, e1))
    if min_d2 is not None:
        min_d2._mvk_min_arg = min_arg          # neighbour column of each minimum: the backward's min_d2 path starts there
    return A, min_d2


def kpconv_scatter(q, s, idx, dA, kp, extent, influence="linear", aggregation="sum", x=None,
                   offsets=None, g_min_d2=None, min_arg=None):
    """dx[idx[n,h],c] += sum_k w[n,h,k] dA[n,k,c]; returns (dx, d_offsets or None)."""
    _dev(q, s, idx, dA, kp)
    q, s, dA, kp = _f32c(q), _f32c(s), _f32c(dA), _f32c(kp)
    idx, i64 = _idx(idx)
    Nq, Ns, H, K, Cin = q.shape[0], s.shape[0], idx.shape[1], kp.shape[0], dA.shape[2]
    dx = _zeros((Ns, Cin), q.device)
    d_off = None
    if offsets is not None:
        offsets, x = _f32c(offsets), _f32c(x)
        # written whole by mvk_kpconv_deform_doff -- which mvk_kpconv_scatter_bwd does not reach for an empty
        # neighbour matrix (its early return): zeros then
        d_off = (torch.zeros if (Nq == 0 or H == 0) else torch.empty)((Nq, K, 3), device=q.device, dtype=torch.float32)
        if g_min_d2 is not None:
            g_min_d2 = _f32c(g_min_d2)
            if min_arg is None:
                raise RuntimeError("kpconv_scatter: the min_d2 gradient needs the forward's arg-min columns")
    check(lib().mvk_kpconv_scatter_bwd(_p(q), Nq, _p(s), Ns, _p(idx), i64, H, Cin, _p(kp), K, float(extent),
                                       INFLUENCE[influence], AGGREGATION[aggregation], _p(dA), _p(dx),
                                       _p(x), _p(offsets), _p(g_min_d2), _p(min_arg), _p(d_off), _stream()))
    return dx, d_off


def kpconv_deform_doff(q, s, idx, x, kp, extent, offsets, dA, g_min_d2=None, min_arg=None):
    """d_offsets [Nq,K,3] of a deformable KPConv alone (mvk_kpconv_deform_doff; kpconv_scatter runs it together with the
    atomic dx scatter): what is left of the scatter entry point once dx is a gather (kpconv_gather_rev_deform)."""
    _dev(q, s, idx, x, kp, offsets, dA, g_min_d2, min_arg)
    q, s, x, kp, offsets, dA = _f32c(q), _f32c(s), _f32c(x), _f32c(kp), _f32c(offsets), _f32c(dA)
    idx, i64 = _idx(idx)
    Nq, Ns, H, K, Cin = q.shape[0], s.shape[0], idx.shape[1], kp.shape[0], dA.shape[2]
    if Nq == 0 or H == 0:
        return torch.zeros((Nq, K, 3), device=q.device, dtype=torch.float32)
    d_off = torch.empty((Nq, K, 3), device=q.device, dtype=torch.float32)
    if g_min_d2 is not None:
        g_min_d2 = _f32c(g_min_d2)
        if min_arg is None:
            raise RuntimeError("kpconv_deform_doff: the min_d2 gradient needs the forward's arg-min columns")
    check(lib().mvk_kpconv_deform_doff(_p(q), Nq, _p(s), Ns, _p(idx), i64, H, _p(x), Cin, _p(kp), K, float(extent),
                                       INFLUENCE["linear"], _p(offsets), _p(dA), _p(g_min_d2), _p(min_arg), _p(d_off),
                                       _stream()))
    return d_off


def kpconv_gather_rev_deform(s, q, rev, g, kp, extent, offsets, modulations=None, order=None):
    """A2 [Ns, K, C]: the forward aggregation of g [Nq, C] over the transposed relation rev [Ns, Hr] with the kernel points
    of the neighbour (query) rows, kp + offsets [Nq,K,3], times modulations [Nq,K] (mvk_kpconv_gather_rev_deform): the
    gather form of a deformable layer's feature gradient, dx = kp_transposed_contraction(A2, W)."""
    _dev(s, q, rev, g, kp, offsets, modulations, order)
    s, q, g, kp, offsets = _f32c(s), _f32c(q), _f32c(g), _f32c(kp), _f32c(offsets)
    if modulations is not None:
        modulations = _f32c(modulations)
    rev, r64 = _idx(rev)
    Ns, Nq, Hr, Cc, K = s.shape[0], q.shape[0], rev.shape[1], g.shape[1], kp.shape[0]
    if rev.shape[0] != Ns or g.shape[0] != Nq or offsets.shape != (Nq, K, 3):
        raise RuntimeError("kpconv_gather_rev_deform: rev [Ns,Hr], g [Nq,C] and offsets [Nq,K,3] expected")
    A2 = torch.empty(Ns * K * Cc + 64, device=s.device, dtype=torch.float32)[:Ns * K * Cc].view(Ns, K, Cc)
    check(lib().mvk_kpconv_gather_rev_deform(_p(s), Ns, _p(q), Nq, _p(rev), r64, Hr, _p(g), Cc, _p(kp), K, float(extent),
                                             _p(offsets), _p(modulations), _p(A2), _p(order), _stream()))
    return A2


# --------------------------------------------------------------------------------------------
# weight-gradient products off the critical chain
# --------------------------------------------------------------------------------------------
# The backward of a layer launches two independent products, dW = A^T g and dA = g W^T; only dA feeds the rest
# of the backward chain, dW is not read before the optimiser. Every product here is a small, latency-bound
# launch (~10 us whatever its size), so all weight gradients of a backward pass run as (at most) two launches:
# `with defer_weight_grads(): loss.backward()`: every dW product of the pass is only RECORDED (its zero-initialised
# result tensor is handed to autograd at once) and the whole list runs as one grouped launch per tile shape when the
# scope ends (mvk_gemm_f32_tn_grouped): ~100 latency-bound ~10 us launches leave the serial chain of a step. Opt-in:
# nothing may read a weight gradient (or accumulate into an existing .grad) before the scope has been left.
_DEFER = {"on": False, "items": [], "leaves": set(), "slots": None, "eager": 0}
_DW_MAX = 512


def _defer_slots(device):
    """Pinned host + device table buffers, allocated outside any capture (pinning is not capturable): two rotate for
    eager passes, every captured pass takes one of its own (its memcpy node re-reads the pinned bytes at each replay)."""
    if _DEFER["slots"] is None:
        nb = _DW_MAX * int(lib().mvk_gemm_group_entry_bytes())
        _DEFER["slots"] = [{"host": torch.empty(nb, dtype=torch.uint8).pin_memory(),
                            "dev": torch.empty(nb, dtype=torch.uint8, device=device), "event": None} for _ in range(34)]
    return _DEFER["slots"]


def capture_table_slots_left(device):
    """Captured passes of defer_weight_grads this process can still record (each keeps one pre-pinned table for good; two
    stay with the eager passes). Ask BEFORE starting a capture: running out inside one raises in the middle of the capture."""
    return max(0, len(_defer_slots(device)) - 2)


class defer_weight_grads:
    """`with defer_weight_grads(): loss.backward()`. flush=False leaves the recorded products to the caller:
    `items = scope.take()` after the block, then `flush_deferred(items, stream)` -- e.g. on a side stream, beside the
    next stage of the backward (bench.py: the weight gradients and the optimiser step of everything above the backward
    cut run while the backward of the point-heavy levels is still computing)."""

    def __init__(self, flush=True):
        self.flush = bool(flush)
        self.items = []

    def __enter__(self):
        _DEFER.update(on=True, items=[], leaves=set())
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                if self.flush:
                    _flush_deferred()
                else:
                    self.items = _DEFER["items"]
        finally:
            _DEFER.update(on=False, items=[], leaves=set())
        return False

    def take(self):
        items, self.items = self.items, []
        return items


def flush_deferred(items, stream=None):
    """The grouped launch for `items` (from defer_weight_grads(flush=False).take()) on `stream` (default: the current
    one). On another stream the operands are marked as used there (record_stream), so their memory is not handed out
    again to work of the producing stream while the grouped product still reads it; the caller orders the streams
    (stream.wait_stream(producer) before, consumer.wait_stream(stream) after)."""
    if not items:
        return
    if stream is None or stream == torch.cuda.current_stream():
        return _flush_deferred(items)
    for it in items:
        it[0].record_stream(stream)
        it[1].record_stream(stream)
    with torch.cuda.stream(stream):
        _flush_deferred(items)


_HAS_USE_COUNT = hasattr(torch._C, "_storage_Use_Count")


def _storage_use_count(storage):
    """Owners of an untyped storage (private torch API, present in the torch 2.x builds this was written against,
    INTEGRATION.md). Without it the deferred mode is not offered at all (_dw_gemm runs every product in line)."""
    return torch._C._storage_Use_Count(storage._cdata)


def _flush_deferred(items=None):
    if items is None:
        items = _DEFER["items"]
    if not items:
        return
    import numpy as np
    dev = items[0][0].device
    n = len(items)
    prob = np.zeros(n, dtype=np.dtype([("A", "<u8"), ("B", "<u8"), ("C", "<u8"), ("M", "<i8"), ("N", "<i8"), ("Kd", "<i8"),
                                       ("ldc", "<i8")]))
    for i, (A, B, out_ptr, _, storage, ldc) in enumerate(items):
        if _storage_use_count(storage) < 2:
            # nothing but this list still owns the result: autograd did not adopt it as a .grad (it added the not yet
            # computed tensor to an existing gradient, or dropped it) -- the product would be lost silently
            raise RuntimeError("defer_weight_grads: a deferred weight-gradient result (%d x %d) was consumed before the "
                               "grouped launch computed it; was the backward run on parameters that already hold a "
                               ".grad, or with hooks that copy gradients? Run it without the scope (MVK_DEFER_DW=0)"
                               % (A.shape[1], B.shape[1]))
        prob[i] = (A.data_ptr(), B.data_ptr(), out_ptr, A.shape[1], B.shape[1], A.shape[0], ldc)
    slots = _defer_slots(dev)
    if torch.cuda.is_current_stream_capturing():
        if len(slots) <= 2:
            raise RuntimeError("defer_weight_grads: out of pre-pinned table slots for graph captures")
        slot = slots.pop()              # owned by this capture from now on
        _DEFER.setdefault("captured", []).append(slot)
    else:
        slot = slots[_DEFER["eager"] % 2]
        _DEFER["eager"] += 1
        if slot["event"] is not None:
            slot["event"].synchronize()
    nn, wn, ww = C.c_int(0), C.c_int64(0), C.c_int64(0)
    splits = np.zeros(n, np.int32)
    check(lib().mvk_gemm_f32_tn_grouped_plan_ldc(prob.ctypes.data_as(C.c_void_p), n, C.c_void_p(slot["host"].data_ptr()),
                                             C.byref(nn), C.byref(wn), C.byref(ww), splits.ctypes.data_as(C.c_void_p),
                                             _stream()))
    for i, item in enumerate(items):
        if splits[i] > 1 and not item[3] and not lib().mvk_gemm_split_ordered():
            raise RuntimeError("defer_weight_grads: the grouped plan splits a product whose output was not zero-initialised")
    nb = n * int(lib().mvk_gemm_group_entry_bytes())
    slot["dev"][:nb].copy_(slot["host"][:nb], non_blocking=True)
    check(lib().mvk_gemm_f32_tn_grouped(C.c_void_p(slot["dev"].data_ptr()), n, nn.value, wn.value, ww.value, _stream()))
    if not torch.cuda.is_current_stream_capturing():
        ev = torch.cuda.Event()
        ev.record()
        slot["event"] = ev


def _accumulate_in_place_ok(t):
    """Whether a backward node may ADD onto its incoming gradient `t` in place (the fan-out sums of _LinearFn /
    _MaxPoolFn). Autograd hands the SAME tensor to every consumer of an addition's gradient (AddBackward, and
    _AddLReLUFn before it returned copies), so `t` may also be an operand of a weight-gradient product that has only
    been RECORDED (defer_weight_grads): mutating it first would corrupt that product silently. Not provably
    exclusive -> the caller computes `product + t` instead."""
    if _DEFER["on"] and _DEFER["items"]:
        # by the bytes the tensors occupy, not by their storages: slices of the zero arena share ONE storage (an operand
        # drawn from it -- the decoder's G_c -- must not make every other arena slice look like an operand)
        if not t.is_contiguous():
            return False
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        for it in _DEFER["items"]:
            for op in (it[0], it[1]):
                a = op.data_ptr()
                if a < hi and lo < a + op.numel() * op.element_size():
                    return False
    return True


def _dw_gemm(A, B, transB=False, target=None):
    """A^T @ B for a weight gradient: deferred into the grouped launch inside defer_weight_grads(), a plain product
    otherwise. `target`: the tensor the gradient is FOR (the Function's weight input). A deferred product hands autograd a result that is only computed when the scope ends, which is
    sound only if AccumulateGrad ADOPTS that tensor as the parameter's .grad: a parameter that already holds a gradient
    (zero_grad(set_to_none=False), micro-batch accumulation, a second backward stage through the same weight) would
    get `grad += <not yet computed>` and the result tensor would be freed before the grouped launch writes it -- such
    products run in line. A weight used twice inside ONE scope cannot be served either way and is refused."""
    leaf = target if (target is not None and target.is_leaf) else None
    if _DEFER["on"] and leaf is not None:
        if id(leaf) in _DEFER["leaves"]:
            raise RuntimeError("defer_weight_grads: the same parameter receives two weight gradients inside one scope "
                               "(shared weights): run this backward without the scope (MVK_DEFER_DW=0)")
        if leaf.grad is not None:
            return gemm(A, B, transA=True, transB=transB)
    if _DEFER["on"] and _HAS_USE_COUNT and not transB and A.is_cuda and B.shape[1] > 16 and len(_DEFER["items"]) < _DW_MAX \
            and A.shape[0] > 0 and A.shape[1] > 0:
        A, B = _f32c(A), _f32c(B)
        # a split reduction accumulates into a zero-initialised output (arena slice); an unsplit one (the big
        # coarse-level weights: few rows to reduce over, 2/3 of all weight-gradient bytes) writes every element
        split_arena_prepare(A.device)
        zeroed = lib().mvk_gemm_f32_tn_grouped_split(A.shape[1], B.shape[1], A.shape[0]) > 1 \
            and not lib().mvk_gemm_split_ordered()
        out = (_zeros((A.shape[1], B.shape[1]), A.device) if zeroed
               else torch.empty((A.shape[1], B.shape[1]), device=A.device, dtype=torch.float32))
        # only the ADDRESS is recorded: a second reference to the tensor would make autograd's AccumulateGrad clone the
        # gradient instead of adopting it (one copy launch per parameter); the tensor itself lives on as the .grad
        # the STORAGE is held too (not a tensor: AccumulateGrad counts tensor references only): its memory cannot be
        # handed out again before the grouped launch has written it, and its owner count tells at flush time whether
        # autograd adopted the result (>= 2) or consumed and dropped it (1)
        # (the last field: the output's leading dimension -- dense here, wider for the slabs of _dw_gemm_slabs)
        _DEFER["items"].append((A, B, out.data_ptr(), zeroed, out.untyped_storage(), B.shape[1]))
        if leaf is not None:
            _DEFER["leaves"].add(id(leaf))
        return out
    return gemm(A, B, transA=True, transB=transB)


def _dw_gemm_slabs(slabs, target=None):
    """[A_0^T B_0 | A_1^T B_1 | ...]: ONE weight gradient whose column slabs are products of their own (the decoder's
    dW = [G_c^T x_c | g^T skip], coarse rows beside fine rows). slabs = [(A_i [Kd_i, M], B_i [Kd_i, n_i])], every Kd_i > 0.
    The rules of _dw_gemm hold for the tensor as a whole: one adopted tensor and one recorded leaf, one table entry per slab
    of more than 16 columns (narrower slabs run in line into their window), zero-initialised when ANY slab's plan splits
    with atomics."""
    leaf = target if (target is not None and target.is_leaf) else None
    defer = _DEFER["on"] and _HAS_USE_COUNT
    if _DEFER["on"] and leaf is not None:
        if id(leaf) in _DEFER["leaves"]:
            raise RuntimeError("defer_weight_grads: the same parameter receives two weight gradients inside one scope "
                               "(shared weights): run this backward without the scope (MVK_DEFER_DW=0)")
        if leaf.grad is not None:
            defer = False
    slabs = [(_f32c(A), _f32c(B)) for A, B in slabs]
    dev, M = slabs[0][0].device, slabs[0][0].shape[1]
    ld = sum(B.shape[1] for _, B in slabs)
    grouped = [defer and B.shape[1] > 16 for _, B in slabs]
    if sum(grouped) + len(_DEFER["items"]) > _DW_MAX:
        grouped = [False] * len(slabs)
    split_arena_prepare(dev)
    ordered = bool(lib().mvk_gemm_split_ordered())
    zeroed = not ordered and any(
        (lib().mvk_gemm_f32_tn_grouped_split(M, B.shape[1], A.shape[0]) if gr else gemm_plan(M, B.shape[1], A.shape[0])[0]) > 1
        for (A, B), gr in zip(slabs, grouped))
    out = _zeros((M, ld), dev) if zeroed else torch.empty((M, ld), device=dev, dtype=torch.float32)
    storage = out.untyped_storage() if any(grouped) else None     # ONE owner for all the slabs (see _dw_gemm, _flush_deferred)
    col0 = 0
    for (A, B), gr in zip(slabs, grouped):
        ptr = out.data_ptr() + 4 * col0
        if gr:
            _DEFER["items"].append((A, B, ptr, zeroed, storage, ld))
        else:
            check(lib().mvk_gemm_f32_tn_ldc(_p(A), _p(B), C.c_void_p(ptr), M, B.shape[1], A.shape[0], ld, _stream()))
        col0 += B.shape[1]
    if any(grouped) and leaf is not None:
        _DEFER["leaves"].add(id(leaf))
    return out


# --------------------------------------------------------------------------------------------
# KPConv (rigid and deformable) as one autograd node
# --------------------------------------------------------------------------------------------

class _KPConvFn(torch.autograd.Function):
    """y = KPConv(q, s, idx, x; kp, W [, offsets, modulations]); also returns min_d2 when deformable.

    Mirrors the tensor algebra of the reference's KPConv.forward
    (KPConv-PyTorch/models/blocks.py:277-374) and its autograd backward."""

    @staticmethod
    def forward(ctx, q, s, idx, x, kp, W, offsets, modulations, extent, influence, aggregation, stats_n_valid=None,
                order=None, rev=None, rev_order=None, finish=None):
        K, Cin, Cout = W.shape
        deform = offsets is not None
        A, min_d2 = kpconv_gather(q, s, idx, x, kp, extent, influence, aggregation, offsets, want_min_d2=deform,
                                  order=order)
        ctx.rev = (rev, rev_order)
        Am = A * modulations.unsqueeze(2) if modulations is not None else A     # blocks.py:366-367
        if _PROF["on"]:
            e0, e1 = _timing_events()
        st = None
        if _contraction_streams(Am, q.shape[0], K * Cin, Cout):                 # the big rigid layers (levels 0-1)
            y, st = gemm_f32_stream(Am.view(-1, K * Cin), W.reshape(K * Cin, Cout), stats_n_valid)
            st = BnStats(*st) if st is not None else None                       # (this kernel finishes nothing)
        else:                                                                   # blocks.py:370-374
            y, st = _product(Am.view(-1, K * Cin), W.reshape(K * Cin, Cout), stats_n_valid=stats_n_valid, finish=finish)
        if _PROF["on"]:
            e1.record()
            _PROF["gemm"].append(((q.shape[0], K * Cin, Cout), e0, e1))
        ctx.save_for_backward(q, s, idx, x, kp, W, A, offsets, modulations)
        ctx.min_arg = getattr(min_d2, "_mvk_min_arg", None)
        ctx.cfg = (extent, influence, aggregation)
        if st is not None:
            ctx.mark_non_differentiable(st.partials)
        ctx.set_materialize_grads(False)    # else autograd hands backward a ZERO tensor (one fill launch) per unused output
        return y, min_d2, st

    @staticmethod
    def backward(ctx, gy, g_min_d2, g_st=None):
        q, s, idx, x, kp, W, A, offsets, modulations = ctx.saved_tensors
        extent, influence, aggregation = ctx.cfg
        K, Cin, Cout = W.shape
        Nq = q.shape[0]
        if gy is None:                      # only min_d2 was used (the regulariser): no feature gradient
            gy = torch.zeros((Nq, Cout), device=q.device, dtype=torch.float32)
        gy = _f32c(gy)
        Am = A * modulations.unsqueeze(2) if modulations is not None else A
        dW = dx = d_off = d_mod = None
        if ctx.needs_input_grad[5]:
            dW = _dw_gemm(Am.view(Nq, K * Cin), gy, target=W).view(K, Cin, Cout)
        need_dA = ctx.needs_input_grad[3] or (offsets is not None)
        rev, rev_order = ctx.rev
        gather_form = (need_dA and rev is not None and REVERSE_DX and rev.shape[0] >= s.shape[0] and Cout >= 5
                       and influence == "linear" and aggregation == "sum")
        if gather_form and rev.shape[0] != s.shape[0]:
            rev = rev[:s.shape[0]]
        if gather_form and offsets is None and modulations is None:
            # gather form (csrc/revlist.hip): the forward kernel over the transposed neighbourhood relation with the
            # kernel points negated, then the per-kernel-point transposed contraction -- no atomics, fixed summation order
            A2, _ = kpconv_gather(s, q, rev, gy, _neg_kernel_points(kp), extent, influence, aggregation, order=rev_order,
                                  tag="[dx]")
            dx = kp_transposed_contraction(A2, W)
        elif need_dA:
            dAm = gemm(gy, W.reshape(K * Cin, Cout), transB=True).view(Nq, K, Cin)
            if modulations is not None:
                if ctx.needs_input_grad[7]:
                    d_mod = (dAm * A).sum(dim=2)
                dA = dAm * modulations.unsqueeze(2)
            else:
                dA = dAm
            if gather_form and offsets is not None:
                # deformable layer (round 5): the same gather with the kernel points -- and modulations -- of the NEIGHBOUR
                # rows (mvk_kpconv_gather_rev_deform); dA is still needed, by the offset gradient and the modulation gradient
                d_off = kpconv_deform_doff(q, s, idx, x, kp, extent, offsets, dA, g_min_d2, ctx.min_arg)
                if ctx.needs_input_grad[3]:
                    A2 = kpconv_gather_rev_deform(s, q, rev, gy, kp, extent, offsets, modulations, order=rev_order)
                    dx = kp_transposed_contraction(A2, W)
            else:
                dx, d_off = kpconv_scatter(q, s, idx, dA, kp, extent, influence, aggregation, x=x,
                                           offsets=offsets,
                                           g_min_d2=g_min_d2 if offsets is not None else None, min_arg=ctx.min_arg)
        return None, None, None, dx, None, dW, d_off, d_mod, None, None, None, None, None, None, None, None


def _contraction_streams(A, M, Kd, N):
    """Whether the forward contraction of a layer runs on gemm_f32_stream: a supported shape and an aggregate with the
    slack the kernel reads behind its last row (kpconv_gather's own allocation has it; a modulated copy does not)."""
    if M <= 0:
        return False
    ok, _, _, need = gemm_f32_stream_plan(M, N, Kd)
    return ok and A.is_contiguous() and _slack_floats(A) >= need


def kpconv(q, s, idx, x, kp, W, extent, influence="linear", aggregation="sum", offsets=None, modulations=None,
           stats_n_valid=None, order=None, rev=None, rev_order=None, bn=None):
    """Returns (y [Nq,Cout], min_d2 [Nq,K] or None). stats_n_valid (DEVICE int32 [1]): the contraction also produces the column statistics
    of y over its first n_valid rows for the BatchNorm that follows (picked up by bn_lrelu via bn_stats_of).
    order (int32 [Nq], a permutation, e.g. neighbors_cell_order of the query level): the order the f32 gather works
    through the query points in (kpconv_gather); the layer's result does not depend on it.
    rev (int32 [Ns, Hr], reverse_neighbors(idx, Ns)) and rev_order (a work list of the SUPPORT level): f32 layers with
    linear influence, sum aggregation and Cout >= 5 then compute the feature gradient as a gather over the transposed
    relation (fixed summation order, no atomics) instead of the atomic scatter.
    bn: the nn.BatchNorm1d that normalises y; its statistics are then FINISHED by the contraction (when _finishable)."""
    if rev is not None and (rev.dtype != torch.int32 or rev.dim() != 2 or not rev.is_contiguous()):
        raise RuntimeError("kpconv: rev must be a contiguous int32 [Ns, Hr] matrix (ops.reverse_neighbors)")
    if influence not in INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation not in AGGREGATION:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    y, min_d2, st = _KPConvFn.apply(q, s, idx, x, kp, W, offsets, modulations, float(extent), influence, aggregation,
                                    stats_n_valid, order, rev, rev_order,
                                    bn if stats_n_valid is not None and _finishable(bn) else None)
    if st is not None:
        y._mvk_bn_stats = st
    return y, min_d2


# --------------------------------------------------------------------------------------------
# offset regulariser of the deformable layers
# --------------------------------------------------------------------------------------------

class _DeformRegFn(torch.autograd.Function):
    """p2p_fitting_regularizer of one deformable KPConv (models/architectures.py:20-58) as one launch that also
    produces both gradients (mvk_deform_regularizer); the backward only scales them by the upstream gradient."""

    @staticmethod
    def forward(ctx, min_d2, deformed_kp, n_valid, extent, repulse_extent, power):
        _dev(min_d2, deformed_kp, n_valid)
        min_d2, dkp = _f32c(min_d2), _f32c(deformed_kp)
        N, K = min_d2.shape
        loss = _zeros((1,), min_d2.device)
        d_min = torch.empty_like(min_d2)
        d_dkp = torch.empty_like(dkp)
        check(lib().mvk_deform_regularizer(_p(min_d2), _p(dkp), _p(n_valid), N, K, float(extent), float(repulse_extent),
                                           float(power), _p(loss), _p(d_min), _p(d_dkp), _stream()))
        ctx.save_for_backward(d_min, d_dkp)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_min, d_dkp = ctx.saved_tensors
        return d_min * g, d_dkp * g, None, None, None, None


class _DeformOperandsFn(torch.autograd.Function):
    """offset_features, offsets, deformed_KP (and modulations) of a deformable KPConv from its inner convolution's
    output (models/blocks.py:243-266, :287), one launch forward and one backward (mvk_deform_operands_fwd/bwd)."""

    @staticmethod
    def forward(ctx, raw, bias, kernel_points, extent, modulated):
        _dev(raw, bias, kernel_points)
        raw, bias, kp = _f32c(raw), _f32c(bias), _f32c(kernel_points)
        N, D = raw.shape
        K = kp.shape[0]
        if D != (4 if modulated else 3) * K or bias.numel() != D:
            raise RuntimeError("deform operands: the inner convolution must deliver %d columns" % ((4 if modulated else 3) * K))
        feat = torch.empty_like(raw)
        offsets = torch.empty((N, K, 3), device=raw.device, dtype=torch.float32)
        dkp = torch.empty_like(offsets)
        mod = torch.empty((N, K), device=raw.device, dtype=torch.float32) if modulated else None
        check(lib().mvk_deform_operands_fwd(_p(raw), _p(bias), _p(kp), N, K, int(bool(modulated)), float(extent), _p(feat),
                                            _p(offsets), _p(dkp), _p(mod), _stream()))
        ctx.save_for_backward(mod)
        ctx.cfg = (N, K, D, float(extent), bool(modulated))
        ctx.set_materialize_grads(False)
        return feat, offsets, dkp, mod

    @staticmethod
    def backward(ctx, g_feat, g_off, g_dkp, g_mod):
        (mod,) = ctx.saved_tensors
        N, K, D, extent, modulated = ctx.cfg
        dev = (mod if mod is not None else next(g for g in (g_feat, g_off, g_dkp, g_mod) if g is not None)).device
        gs = [None if g is None else _f32c(g) for g in (g_off, g_dkp, g_mod, g_feat)]
        d_raw = torch.empty((N, D), device=dev, dtype=torch.float32)
        d_bias = _zeros((D,), dev)
        check(lib().mvk_deform_operands_bwd(_p(gs[0]), _p(gs[1]), _p(gs[2]), _p(mod), _p(gs[3]), N, K, int(modulated), extent,
                                            _p(d_raw), _p(d_bias), _stream()))
        return d_raw, d_bias, None, None, None


def deform_operands(raw, bias, kernel_points, extent, modulated=False):
    """(offset_features [N,D], offsets [N,K,3], deformed_KP [N,K,3], modulations [N,K] or None) from the inner
    convolution's output raw [N,D] (D = 3K, 4K when modulated)."""
    return _DeformOperandsFn.apply(raw, bias, kernel_points, extent, modulated)


def _reg_many(cfgs, ts, grads, loss, gscale):
    """mvk_deform_regularizer_many over the layers (min_d2, deformed_kp) = ts[2i], ts[2i+1], REG_MANY per launch (layers
    of another K get their own launch)."""
    from ._lib import RegLayer
    by_k = {}
    for i, (extent, repulse, power, nv) in enumerate(cfgs):
        m, d = ts[2 * i], ts[2 * i + 1]
        L = RegLayer(_p(m), _p(d), _p(nv), _p(grads[2 * i]) if grads else None, _p(grads[2 * i + 1]) if grads else None,
                     m.shape[0], float(extent), float(repulse), float(power))
        by_k.setdefault(int(m.shape[1]), []).append(L)
    for K, layers in by_k.items():
        for b in range(0, len(layers), REG_MANY):
            part = layers[b:b + REG_MANY]
            arr = (RegLayer * len(part))(*part)
            check(lib().mvk_deform_regularizer_many(arr, len(part), K, _p(loss), _p(gscale), _stream()))


class _DeformRegAllFn(torch.autograd.Function):
    """The regulariser terms of ALL deformable layers of a network as one autograd node: every layer's forward launch
    accumulates into one scalar (no additions of per-layer losses), the backward launches the same kernel with the
    upstream gradient as a device scalar and gets both gradients already scaled (no multiplications)."""

    @staticmethod
    def forward(ctx, cfgs, *tensors):
        ts = [_f32c(t) for t in tensors]
        _dev(*ts)
        loss = _zeros((1,), ts[0].device)
        _reg_many(cfgs, ts, None, loss, None)
        ctx.save_for_backward(*ts)
        ctx.cfgs = cfgs
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        ts = ctx.saved_tensors
        g = _f32c(g).reshape(1)
        grads = [torch.empty_like(t) for t in ts]
        _reg_many(ctx.cfgs, ts, grads, None, g)
        return (None, *grads)


def deform_regularizer_all(layers):
    """Sum of the regulariser terms of several deformable layers; layers: list of (min_d2 [N,K], deformed_kp [N,K,3],
    extent, repulse_extent, power, n_valid or None). Layers without rows contribute nothing."""
    layers = [l for l in layers if l[0].shape[0] > 0]
    if not layers:
        return None
    cfgs = [(l[2], l[3], l[4], l[5]) for l in layers]
    flat = []
    for l in layers:
        flat += [l[0], l[1]]
    return _DeformRegAllFn.apply(cfgs, *flat)


def deform_regularizer(min_d2, deformed_kp, extent, repulse_extent, power=1.0, n_valid=None):
    """power * (2 * fitting + repulsive) of one deformable layer; min_d2 [N,K], deformed_kp [N,K,3]; n_valid: DEVICE
    int32 [1] row count of a capacity-padded level (means over the valid rows only) or None."""
    return _DeformRegFn.apply(min_d2, deformed_kp, n_valid, extent, repulse_extent, power)


# --------------------------------------------------------------------------------------------
# masked BatchNorm + LeakyReLU (capacity-padded levels, hipGraph replay)
# --------------------------------------------------------------------------------------------

# capacity-padded mode: {row capacity of a level: DEVICE int32[1] tensor holding the valid row count}.
# Set by the network wrapper around a forward pass (see synthetic.CapacityBatch); empty = plain mode.
_ROW_COUNTS = {}


def set_row_counts(mapping):
    _ROW_COUNTS.clear()
    if mapping:
        _ROW_COUNTS.update(mapping)


def row_count_for(rows):
    return _ROW_COUNTS.get(int(rows))


_COUNT_TABLE = {}                    # device index -> int32 [0, 1, 2, ...]: word r of it holds the value r, for good
_COUNT_TABLE_ROWS = 1 << 22
_BIG_COUNTS = {}                     # (rows, device index) beyond the table: one word each, never freed


def full_count(rows, device):
    """Device int32 [1] holding `rows`: the n_valid of a tensor without padded rows. A view of word `rows` of a constant
    table [0, 1, 2, ...] (16 MB per device, written ONCE by an eager launch): no fill launch per call, no
    host-to-device copy, nothing to evict, and the same word is valid in eager code and in every captured graph -- the
    row count of every pyramid level changes with each batch in ordinary training. The table cannot be created while a
    stream is capturing (its fill would become a node of that graph and the words would be undefined for everyone
    else until that graph has replayed): any eager step before the capture creates it, or full_count_prepare()."""
    rows = int(rows)
    t = _COUNT_TABLE.get(device.index)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ops.full_count: the constant row-count table does not exist yet and cannot be created "
                               "inside a graph capture; run one eager step first or call ops.full_count_prepare(device)")
        t = torch.arange(_COUNT_TABLE_ROWS, dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()      # other streams read views of it without any event
        _COUNT_TABLE[device.index] = t
    if 0 <= rows < _COUNT_TABLE_ROWS:
        return t[rows:rows + 1]
    key = (rows, device.index)
    w = _BIG_COUNTS.get(key)
    if w is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ops.full_count: %d rows lie beyond the constant table; request this count once outside "
                               "the capture" % rows)
        w = torch.full((1,), rows, dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()
        _BIG_COUNTS[key] = w
    return w


def full_count_prepare(device):
    """Creates the constant table of full_count() (call before capturing a graph that was never run eagerly)."""
    full_count(0, torch.device(device))


def _bn_fwd_problem(who, x, n_valid, gamma, beta, running_mean, running_var, cfg, nbt, addend, ext):
    """The arguments of mvk_bn_lrelu_fwd for x [R,D] (f32, contiguous) in the order of the export and of the fields of
    mvk_bn_fwd_problem, cfg = (eps, momentum, slope), ext = the input's BnStats (bn_stats_of) or None; then y, mean, invstd and
    whatever else must stay alive until the launch has been issued."""
    R, D = x.shape
    y = torch.empty_like(x)
    ext_part, ext_rows, fin = ext if ext is not None else (None, 0, None)
    if ext_part is not None and (ext_part.shape[2] != D or ext_part.shape[0] != (R + ext_rows - 1) // ext_rows):
        raise RuntimeError("%s: the statistics partials do not belong to this tensor" % who)
    scratch = None
    if fin is not None:
        # statistics finished by the producing product (mean, invstd, running statistics, batch counter): apply only
        mean, invstd = fin
        running_mean = running_var = nbt = ext_part = None
        ext_rows = -1
    else:
        mean = torch.empty(D, device=x.device, dtype=torch.float32)
        invstd = torch.empty(D, device=x.device, dtype=torch.float32)
        if ext_part is None:
            scratch = torch.empty(((R + 63) // 64) * 2 * D, device=x.device, dtype=torch.float32)
    eps, momentum, slope = cfg
    args = (_p(x), _p(n_valid), R, D, _p(gamma), _p(beta), float(eps), float(momentum), float(slope), _p(running_mean),
            _p(running_var), _p(mean), _p(invstd), _p(scratch), _p(y), _p(nbt), _p(addend), _p(ext_part), int(ext_rows))
    return args, y, mean, invstd, scratch


def _bn_bwd_problem(x, g, n_valid, gamma, beta, mean, invstd, slope, yout):
    """The arguments of mvk_bn_lrelu_bwd (= the fields of mvk_bn_bwd_problem) for the upstream gradient g; then
    dgamma_dbeta [2D] (dbeta, then dgamma), dx, the addend's gradient (None without yout) and what must stay alive."""
    g = _f32c(g)
    R, D = x.shape
    dgb = torch.empty(2 * D, device=x.device, dtype=torch.float32)
    scratch = torch.empty(((R + 63) // 64) * 2 * D, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    d_add = torch.empty_like(x) if yout is not None else None
    args = (_p(x), _p(g), _p(n_valid), R, D, _p(gamma), _p(beta), _p(mean), _p(invstd), float(slope), _p(scratch), _p(dgb),
            _p(dx), _p(yout), _p(d_add))
    return args, dgb, dx, d_add, (g, scratch)


class _BNLReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_valid, gamma, beta, running_mean, running_var, eps, momentum, slope, training, nbt=None,
                addend=None, ext=None):
        _dev(x, n_valid, gamma, beta, addend)
        x = _f32c(x)
        if addend is not None:
            addend = _f32c(addend)
            if addend.shape != x.shape:
                raise RuntimeError("bn_lrelu: the residual addend must have the shape of the input")
        if not training:
            raise RuntimeError("masked BatchNorm is a training-mode op; use nn.BatchNorm1d in eval mode")
        args, y, mean, invstd, _keep = _bn_fwd_problem("bn_lrelu", x, n_valid, gamma, beta, running_mean, running_var,
                                                       (eps, momentum, slope), nbt, addend, ext)
        check(lib().mvk_bn_lrelu_fwd(*args, _stream()))
        ctx.save_for_backward(x, n_valid, gamma, beta, mean, invstd, y if addend is not None else None)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, g):
        x, n_valid, gamma, beta, mean, invstd, yout = ctx.saved_tensors
        args, dgb, dx, d_add, _keep = _bn_bwd_problem(x, g, n_valid, gamma, beta, mean, invstd, ctx.slope, yout)
        check(lib().mvk_bn_lrelu_bwd(*args, _stream()))
        D = x.shape[1]
        return dx, None, dgb[D:], dgb[:D], None, None, None, None, None, None, None, d_add, None


# ---- synchronised BatchNorm (opt-in; SURVEY.md 8e, models/blocks.py:453-460) --------------------------------------
# The reference normalises over the stacked point axis of the WHOLE batch. Sharding the spheres over ranks leaves every
# rank the statistics of its own spheres (the default, a documented deviation); with set_sync_batchnorm(group) the
# statistics of every BatchNorm -- blocks and FeatureAggregation alike -- are those of all ranks' rows: N ranks x S
# spheres then compute what one rank x N*S spheres computes (tests/test_model_gpu.py, two ranks). Written with
# differentiable tensor ops and torch.distributed.nn's differentiable all-reduce (two all-reduces of C floats forward,
# their mirror images backward): an option for runs that must match a single-GPU run, not a tuned path.
_SYNC_BN = {"group": None}


def set_sync_batchnorm(group):
    """group: a torch.distributed process group, True (the default group) or None (per-rank statistics: the default)."""
    if group is True:
        import torch.distributed as dist
        group = dist.group.WORLD
    _SYNC_BN["group"] = group


def _sync_bn_lrelu(x, n_valid, bn, slope, addend):
    import torch.distributed as dist
    from torch.distributed.nn.functional import all_reduce
    group = _SYNC_BN["group"]
    if not bn.training:
        raise RuntimeError("synchronised BatchNorm is a training-mode op; use nn.BatchNorm1d in eval mode")
    x = _f32c(x)
    R, D = x.shape
    mask = (torch.arange(R, device=x.device) < n_valid.to(torch.int64)).to(x.dtype).unsqueeze(1)     # valid rows
    n = all_reduce(n_valid.to(x.dtype).reshape(1), op=dist.ReduceOp.SUM, group=group)
    mean = all_reduce((x * mask).sum(0), op=dist.ReduceOp.SUM, group=group) / n
    d = (x - mean) * mask
    var = all_reduce((d * d).sum(0), op=dist.ReduceOp.SUM, group=group) / n                          # biased, about the GLOBAL mean
    y = d * torch.rsqrt(var + bn.eps) * bn.weight + bn.bias
    if addend is not None:
        y = y + addend
    y = torch.nn.functional.leaky_relu(y, slope) if slope != 1.0 else y
    y = y * mask
    if bn.track_running_stats:
        with torch.no_grad():
            m = bn.momentum if bn.momentum is not None else 0.0
            bn.running_mean.mul_(1 - m).add_(m * mean.detach())
            bn.running_var.mul_(1 - m).add_(m * var.detach() * (n / (n - 1).clamp(min=1)))
            bn.num_batches_tracked += 1
    return y


def bn_lrelu(x, n_valid, bn, slope=1.0, addend=None):
    """y = LeakyReLU_slope(BatchNorm1d(x[:n_valid]) [+ addend]) with rows >= n_valid zeroed; `bn` is an
    nn.BatchNorm1d whose parameters / running statistics are used and updated; n_valid is a DEVICE
    int32 tensor of one element. addend [R,D]: the shortcut of a residual block, joined before the
    activation (blocks.py:649) inside the same launch; it receives its own gradient."""
    if _SYNC_BN["group"] is not None:
        return _sync_bn_lrelu(x, n_valid, bn, slope, addend)
    nbt = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None   # += 1 inside the kernel
    return _BNLReLUFn.apply(x, n_valid, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                            bn.momentum if bn.momentum is not None else 0.0, slope, bn.training, nbt, addend,
                            bn_stats_of(x))


class _BNLazyFn(torch.autograd.Function):
    """y = LeakyReLU_slope(BatchNorm(x)) with FINISHED statistics whose forward launches nothing: the product that consumes
    y applies the transform while it stages its A operand and writes y on the way (mvk_a_transform, bn_lrelu_linear).
    The backward is the masked BatchNorm's own (_BNLReLUFn.backward without an addend)."""

    @staticmethod
    def forward(ctx, x, n_valid, gamma, beta, mean, invstd, slope):
        y = torch.empty_like(x)
        ctx.save_for_backward(x, n_valid, gamma, beta, mean, invstd)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, g):
        x, n_valid, gamma, beta, mean, invstd = ctx.saved_tensors
        args, dgb, dx, _, _keep = _bn_bwd_problem(x, g, n_valid, gamma, beta, mean, invstd, ctx.slope, None)
        check(lib().mvk_bn_lrelu_bwd(*args, _stream()))
        D = x.shape[1]
        return dx, None, dgb[D:], dgb[:D], None, None, None


XF_KMAX = 512        # csrc/gemm.hip: longest reduction a product with an operand transform takes


def bn_lrelu_linear(x, n_valid, bn, slope, W, stats_n_valid=None, bn_out=None):
    """linear(bn_lrelu(x, n_valid, bn, slope), W, stats_n_valid=..., bn=bn_out) with the BatchNorm's apply pass folded
    into the product's operand load (blocks.py:639-644: batch_norm_conv + LeakyReLU + unary2): x must carry statistics
    FINISHED by its producer (kpconv(..., bn=bn) / linear(..., bn=bn)). Returns (y, activations) -- the activations are
    the tensor bn_lrelu would have returned, written by the product -- or None when the fold does not apply (the caller
    then runs the two steps)."""
    fin = getattr(bn_stats_of(x), "finished", None)
    R, Kd = x.shape
    if (fin is None or not BN_FOLD or _SYNC_BN["group"] is not None or not x.is_cuda or x.dtype != torch.float32
            or not x.is_contiguous() or W.dtype != torch.float32 or not W.is_contiguous() or W.shape[1] != Kd
            or W.shape[0] <= 32 or Kd > XF_KMAX or Kd % 4 != 0 or R == 0 or not slope > 0):
        return None
    mean, invstd = fin
    lazy = _BNLazyFn.apply(x, n_valid, bn.weight, bn.bias, mean, invstd, float(slope))
    xf = {"raw": x.detach(), "mean": mean, "invstd": invstd, "gamma": bn.weight.detach(), "beta": bn.bias.detach(),
          "slope": float(slope), "n_valid": n_valid, "lazy": lazy}
    return linear(lazy, W, stats_n_valid=stats_n_valid, bn=bn_out, _a_transform=xf), lazy


class _BNLReLUPairFn(torch.autograd.Function):
    """Two masked BatchNorm (+ LeakyReLU) problems of the same row count, one launch each way (mvk_bn_lrelu_fwd_pair /
    _bwd_pair): the convolution output and the shortcut of a bottleneck block. No residual addend in either."""

    @staticmethod
    def forward(ctx, xa, xb, n_valid, ga, ba, rma, rva, gb, bb, rmb, rvb, cfg_a, cfg_b, nbt_a, nbt_b, ext_a, ext_b):
        from ._lib import BnFwdProblem
        _dev(xa, xb, n_valid, ga, ba, gb, bb)
        xa, xb = _f32c(xa), _f32c(xb)
        if xa.shape[0] != xb.shape[0]:
            raise RuntimeError("bn_lrelu_pair: the two inputs differ in rows")
        (args_a, ya, mean_a, is_a, _ka), (args_b, yb, mean_b, is_b, _kb) = [
            _bn_fwd_problem("bn_lrelu_pair", x, n_valid, g, b, rm, rv, cfg, nbt, None, ext)
            for x, g, b, rm, rv, cfg, nbt, ext in ((xa, ga, ba, rma, rva, cfg_a, nbt_a, ext_a),
                                                   (xb, gb, bb, rmb, rvb, cfg_b, nbt_b, ext_b))]
        check(lib().mvk_bn_lrelu_fwd_pair(C.byref(BnFwdProblem(*args_a)), C.byref(BnFwdProblem(*args_b)), _stream()))
        ctx.save_for_backward(xa, xb, n_valid, ga, ba, gb, bb, mean_a, is_a, mean_b, is_b)
        ctx.slopes = (float(cfg_a[2]), float(cfg_b[2]))
        ctx.set_materialize_grads(False)
        return ya, yb

    @staticmethod
    def backward(ctx, g_a, g_b):
        from ._lib import BnBwdProblem
        xa, xb, n_valid, ga, ba, gb, bb, mean_a, is_a, mean_b, is_b = ctx.saved_tensors
        (args_a, dgb_a, dx_a, _, _ka), (args_b, dgb_b, dx_b, _, _kb) = [
            _bn_bwd_problem(x, g if g is not None else torch.zeros_like(x), n_valid, gam, bet, mean, istd, slope, None)
            for x, g, gam, bet, mean, istd, slope in ((xa, g_a, ga, ba, mean_a, is_a, ctx.slopes[0]),
                                                      (xb, g_b, gb, bb, mean_b, is_b, ctx.slopes[1]))]
        check(lib().mvk_bn_lrelu_bwd_pair(C.byref(BnBwdProblem(*args_a)), C.byref(BnBwdProblem(*args_b)), _stream()))
        Da, Db = xa.shape[1], xb.shape[1]
        return (dx_a, dx_b, None, dgb_a[Da:], dgb_a[:Da], None, None, dgb_b[Db:], dgb_b[:Db], None, None, None, None, None,
                None, None, None)


def bn_lrelu_pair(xa, bn_a, slope_a, xb, bn_b, slope_b, n_valid):
    """(bn_lrelu(xa, n_valid, bn_a, slope_a), bn_lrelu(xb, n_valid, bn_b, slope_b)) as ONE launch each way: two inputs of
    the same row count normalised independently (the convolution and the shortcut of a bottleneck block)."""
    def unpack(bn):
        nbt = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None
        return nbt, (bn.eps, bn.momentum if bn.momentum is not None else 0.0)
    if not (bn_a.training and bn_b.training):
        raise RuntimeError("masked BatchNorm is a training-mode op; use nn.BatchNorm1d in eval mode")
    if _SYNC_BN["group"] is not None:
        return _sync_bn_lrelu(xa, n_valid, bn_a, slope_a, None), _sync_bn_lrelu(xb, n_valid, bn_b, slope_b, None)
    nbt_a, (eps_a, mom_a) = unpack(bn_a)
    nbt_b, (eps_b, mom_b) = unpack(bn_b)
    return _BNLReLUPairFn.apply(xa, xb, n_valid, bn_a.weight, bn_a.bias, bn_a.running_mean, bn_a.running_var,
                                bn_b.weight, bn_b.bias, bn_b.running_mean, bn_b.running_var,
                                (eps_a, mom_a, slope_a), (eps_b, mom_b, slope_b), nbt_a, nbt_b,
                                bn_stats_of(xa), bn_stats_of(xb))


class _AddLReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, slope):
        _dev(a, b)
        a, b = _f32c(a), _f32c(b)
        y = torch.empty_like(a)
        check(lib().mvk_add_lrelu_fwd(_p(a), _p(b), a.numel(), float(slope), _p(y), _stream()))
        ctx.save_for_backward(y)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _f32c(g)
        d = torch.empty_like(y)
        check(lib().mvk_add_lrelu_bwd(_p(y), _p(g), y.numel(), ctx.slope, _p(d), _stream()))
        # two DISTINCT tensors: downstream nodes accumulate onto their incoming gradient in place (_LinearFn, _MaxPoolFn)
        # or record it as the operand of a deferred product -- one buffer for both branches would alias them
        return d, d.clone(), None


def _bias_grad(y):
    """Buffer for the bias gradient of mvk_bias_lrelu_bwd: it becomes the .grad of a leaf parameter, so it is never a
    slice of the per-step zero arena; written whole by the ordered reduction, zero-initialised otherwise."""
    split_arena_prepare(y.device)
    if lib().mvk_gemm_split_ordered():
        return torch.empty((y.shape[1],), device=y.device, dtype=torch.float32)
    return torch.zeros((y.shape[1],), device=y.device, dtype=torch.float32)


class _BiasLReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, slope):
        _dev(x, bias)
        x, bias = _f32c(x), _f32c(bias)
        y = torch.empty_like(x)
        check(lib().mvk_bias_lrelu_fwd(_p(x), _p(bias), x.shape[0], x.shape[1], float(slope), _p(y), _stream()))
        ctx.save_for_backward(y)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _f32c(g)
        dx = torch.empty_like(y)
        db = _bias_grad(y)
        check(lib().mvk_bias_lrelu_bwd(_p(y), _p(g), y.shape[0], y.shape[1], ctx.slope, _p(dx), _p(db), _stream()))
        return dx, db, None


def bias_lrelu(x, bias, slope=0.1):
    """LeakyReLU_slope(x + bias) for [R, C <= 256] rows in one launch each way (blocks.py:462-463 + the block's
    LeakyReLU; slope = 1: the bias alone). slope must be positive (the backward reads the sign from the output)."""
    if x.dim() != 2 or bias.dim() != 1 or bias.shape[0] != x.shape[1]:
        raise RuntimeError("bias_lrelu: x [R,C] and bias [C] expected")
    if not slope > 0:
        raise ValueError("bias_lrelu: slope must be positive")
    return _BiasLReLUFn.apply(x, bias, slope)


class _LinearBiasActFn(torch.autograd.Function):
    """LeakyReLU_slope(x W^T + bias) with the bias and the activation in the GEMM's store (mvk_gemm_f32_bias_act); the
    backward is bias_lrelu's (mask from the saved output, bias gradient in the same launch) followed by the layer's two
    products."""

    @staticmethod
    def forward(ctx, x, W, bias, slope):
        _dev(x, W, bias)
        x, W, bias = _f32c(x), _f32c(W), _f32c(bias)
        y = torch.empty((x.shape[0], W.shape[0]), device=x.device, dtype=torch.float32)
        if x.shape[0] > 0:
            check(lib().mvk_gemm_f32_bias_act(_p(x), _p(W), _p(y), x.shape[0], W.shape[0], x.shape[1], 1, _p(bias),
                                              float(slope), _stream()))
        ctx.save_for_backward(x, W, y)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W, y = ctx.saved_tensors
        g = _f32c(g)
        d = torch.empty_like(y)
        db = _bias_grad(y)
        check(lib().mvk_bias_lrelu_bwd(_p(y), _p(g), y.shape[0], y.shape[1], ctx.slope, _p(d), _p(db), _stream()))
        dx = gemm(d, W) if ctx.needs_input_grad[0] else None
        dW = _dw_gemm(d, x, target=W) if ctx.needs_input_grad[1] else None
        return dx, dW, db, None


def linear_bias_lrelu(x, W, bias, slope=0.1):
    """bias_lrelu(linear(x, W), bias, slope) in one launch forward (a BatchNorm-less UnaryBlock: the head layers)."""
    if x.dim() != 2 or bias.dim() != 1 or bias.shape[0] != W.shape[0] or W.shape[1] != x.shape[1]:
        raise RuntimeError("linear_bias_lrelu: x [R,K], W [C,K] and bias [C] expected")
    if not slope > 0:
        raise ValueError("linear_bias_lrelu: slope must be positive")
    return _LinearBiasActFn.apply(x, W, bias, slope)


def add_lrelu(a, b, slope=0.1):
    """LeakyReLU(a + b) in one launch (residual join of ResnetBottleneckBlock, blocks.py:649)."""
    if a.shape != b.shape:
        raise RuntimeError("add_lrelu: shapes differ")
    return _AddLReLUFn.apply(a, b, slope)


# --------------------------------------------------------------------------------------------
# pooling helpers of blocks.py
# --------------------------------------------------------------------------------------------

class _MaxPoolFn(torch.autograd.Function):
    """passthrough (see _LinearFn): a second, aliasing output of x for another consumer of x; the backward scatters onto
    that consumer's gradient (the kernel accumulates with atomics anyway) instead of onto zeros + one more add."""

    @staticmethod
    def forward(ctx, x, inds, passthrough=False):
        _dev(x, inds)
        x = _f32c(x)
        ctx.rev = reverse_for(inds) if is_deterministic() else None       # (by the batch's own tensor object)
        inds, i64 = _idx(inds)
        Nq, H = inds.shape
        out = torch.empty((Nq, x.shape[1]), device=x.device, dtype=torch.float32)
        arg = torch.empty((Nq, x.shape[1]), device=x.device, dtype=torch.int32)
        check(lib().mvk_max_pool_fwd(_p(x), x.shape[0], x.shape[1], _p(inds), i64, Nq, H, _p(out), _p(arg), _stream()))
        ctx.save_for_backward(inds, arg)
        ctx.ns, ctx.c = x.shape[0], x.shape[1]
        ctx.set_materialize_grads(False)
        return out, (x.view_as(x) if passthrough else None)

    @staticmethod
    def backward(ctx, g, g_alias=None):
        inds, arg = ctx.saved_tensors
        if g is None:
            return g_alias, None, None
        g = _f32c(g)
        if is_deterministic():
            rev = ctx.rev
            if rev is not None and rev.shape[0] >= ctx.ns:
                base = g_alias if (g_alias is not None and g_alias.shape == (ctx.ns, ctx.c)) else None
                dx = torch.empty((ctx.ns, ctx.c), device=g.device, dtype=torch.float32)
                check(lib().mvk_max_pool_bwd_gather(_p(g), _p(arg), _p(inds), int(inds.dtype == torch.int64), inds.shape[1],
                                                    inds.shape[0], _p(rev), rev.shape[1], ctx.ns, ctx.c,
                                                    _p(_f32c(base)) if base is not None else None, _p(dx), _stream()))
                if g_alias is not None and base is None:
                    dx = dx + g_alias
                return dx, None, None
            _no_reverse_list("a max_pool matrix")
        if (g_alias is not None and g_alias.dtype == torch.float32 and g_alias.is_contiguous()
                and g_alias.shape == (ctx.ns, ctx.c) and _accumulate_in_place_ok(g_alias)):
            dx = g_alias            # this node's own grad input, not an operand of a pending product
        else:
            dx = _zeros((ctx.ns, ctx.c), g.device)
        check(lib().mvk_max_pool_bwd(_p(g), _p(arg), _p(inds), int(inds.dtype == torch.int64), inds.shape[0],
                                     inds.shape[1], ctx.ns, g.shape[1], _p(dx), _stream()))
        if g_alias is not None and dx is not g_alias:
            dx = dx + g_alias
        return dx, None, None


class _GatherRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inds2d):
        _dev(x, inds2d)
        x = _f32c(x)
        ctx.rev = reverse_for(inds2d, first_column=True) if is_deterministic() else None
        inds2d, i64 = _idx(inds2d)
        Nq = inds2d.shape[0]
        stride = inds2d.shape[1] if inds2d.dim() == 2 else 1
        out = torch.empty((Nq, x.shape[1]), device=x.device, dtype=torch.float32)
        check(lib().mvk_gather_rows_fwd(_p(x), x.shape[0], x.shape[1], _p(inds2d), i64, Nq, stride, _p(out), _stream()))
        ctx.save_for_backward(inds2d)
        ctx.ns, ctx.stride = x.shape[0], stride
        return out

    @staticmethod
    def backward(ctx, g):
        (inds2d,) = ctx.saved_tensors
        # a column slice of a wider gradient (one half of the decoder's concatenation) is read in place
        if not (g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1 and g.stride(0) >= g.shape[1]):
            g = _f32c(g)
        if is_deterministic():
            rev = ctx.rev
            if rev is not None and rev.shape[0] >= ctx.ns:
                return gather_sum_rows(g, rev[:ctx.ns]), None
            _no_reverse_list("a closest_pool / upsampling matrix")
        dx = _zeros((ctx.ns, g.shape[1]), g.device)
        check(lib().mvk_gather_rows_bwd_ld(_p(g), g.stride(0), _p(inds2d), int(inds2d.dtype == torch.int64),
                                           inds2d.shape[0], ctx.stride, ctx.ns, g.shape[1], _p(dx), _stream()))
        return dx, None


class _UpsampleCatFn(torch.autograd.Function):
    """[closest_pool(x, inds) | skip] in one launch (mvk_gather_rows_cat_fwd); the backward reads the upsampled half of
    the gradient in place (as _GatherRowsFn does behind torch.cat) and hands the skip half on as a view."""

    @staticmethod
    def forward(ctx, x, inds2d, skip):
        _dev(x, inds2d, skip)
        x, skip = _f32c(x), _f32c(skip)
        ctx.rev = reverse_for(inds2d, first_column=True) if is_deterministic() else None
        inds2d, i64 = _idx(inds2d)
        Nq = inds2d.shape[0]
        if skip.shape[0] != Nq:
            raise RuntimeError("upsample_cat: the skip features and the upsampling indices differ in length")
        stride = inds2d.shape[1] if inds2d.dim() == 2 else 1
        C1, C2 = x.shape[1], skip.shape[1]
        out = torch.empty((Nq, C1 + C2), device=x.device, dtype=torch.float32)
        check(lib().mvk_gather_rows_cat_fwd(_p(x), x.shape[0], C1, _p(inds2d), i64, Nq, stride, _p(skip), C2, _p(out),
                                            _stream()))
        ctx.save_for_backward(inds2d)
        ctx.ns, ctx.stride, ctx.c1 = x.shape[0], stride, C1
        return out

    @staticmethod
    def backward(ctx, g):
        (inds2d,) = ctx.saved_tensors
        g = _f32c(g)
        c2 = g.shape[1] - ctx.c1
        if is_deterministic():
            rev = ctx.rev
            if rev is not None and rev.shape[0] >= ctx.ns:
                dx = gather_sum_rows(g[:, :ctx.c1], rev[:ctx.ns]) if ctx.needs_input_grad[0] else None
                return dx, None, (g[:, ctx.c1:].contiguous() if ctx.needs_input_grad[2] else None)
            _no_reverse_list("a closest_pool / upsampling matrix")
        dx = _zeros((ctx.ns, ctx.c1), g.device) if ctx.needs_input_grad[0] else None
        # the skip half leaves as a dense tensor of its own (same launch): the encoder block that produced the skip
        # features accumulates its own gradient onto it (max_pool / linear passthrough) instead of a separate add
        d_skip = torch.empty((g.shape[0], c2), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        check(lib().mvk_gather_rows_cat_bwd(_p(g), _p(inds2d), int(inds2d.dtype == torch.int64), inds2d.shape[0],
                                            ctx.stride, ctx.ns, ctx.c1, c2, _p(dx), _p(d_skip), _stream()))
        return dx, None, d_skip


# The decoder's unary layers as two products: by linearity
#   cat([x_c[idx], skip]) . W^T = (x_c . W[:, :C1]^T)[idx] + skip . W[:, C1:]^T
# so the upsampled half is multiplied at COARSE rows (every level keeps ~1/4.4 of the points) and the concatenation is
# never built. MVK_DECODER_SPLIT=0 (or ops.DECODER_SPLIT = False) keeps the concatenated form.
DECODER_SPLIT = os.environ.get("MVK_DECODER_SPLIT", "1") != "0"


def _nt_ldb_add(A, W, col0, Kd, addend=None, stats_n_valid=None, finish=None):
    """A [M,Kd] . W[:, col0:col0+Kd]^T (+ src[idx[m]] for addend = (src [ns,N], idx, i64, stride)) with the statistics
    epilogue / finish of _product (mvk_gemm_f32_nt_ldb_add): returns (C, BnStats or None)."""
    M, N = A.shape[0], W.shape[0]
    split_arena_prepare(A.device)
    stats_ok = stats_n_valid is not None and M <= _STATS_EPILOGUE_ROWS
    if finish is None:
        stats_ok = stats_ok and M > bn_single_launch_rows(N)
    split, rows = gemm_plan(M, N, Kd, None, stats_ok)
    out = _split_out((M, N), A.device, split)
    part = torch.empty(((M + rows - 1) // rows, 2, N), device=A.device, dtype=torch.float32) if rows > 0 else None
    fin = done = None
    if finish is not None and part is not None:
        fin, done = _fin_struct(finish, N, A.device)
    src, idx, i64, stride = addend if addend is not None else (None, None, 0, 1)
    check(lib().mvk_gemm_f32_nt_ldb_add(_p(A), _p(W), int(col0), W.shape[1], _p(out), M, N, int(Kd), _p(src), _p(idx), int(i64),
                                        int(stride), src.shape[0] if src is not None else 0, _p(part),
                                        _p(stats_n_valid) if part is not None else None,
                                        C.byref(fin) if fin is not None else None, _stream()))
    return out, (BnStats(part, rows, done) if part is not None else None)


class _UpsampleCatLinearFn(torch.autograd.Function):
    """linear(cat([closest_pool(x, inds), skip], 1), W): the decoder's upsampling, concatenation and unary layer.
    Split form (DECODER_SPLIT, the default): forward Yc = x W[:, :C1]^T at coarse rows, then y = skip W[:, C1:]^T + Yc[idx]
    with the statistics epilogue as in linear() -- two launches, no concatenation. Backward: G_c = the gradient rows summed
    per coarse point, then dx = G_c W[:, :C1] and d_skip = g W[:, C1:] in one pair launch, dW = [G_c^T x | g^T skip] as two
    deferred products into one tensor.
    Concatenated form: the fused gather + concatenation, then the GEMM. Backward: ONE product for both
    inputs -- g W is never stored, the GEMM's epilogue scatters its upsampled columns onto dx and writes the skip columns
    (mvk_gemm_f32_scatter_cat) -- and the weight gradient from the saved concatenation."""

    @staticmethod
    def forward(ctx, x, inds2d, skip, W, stats_n_valid, finish=None):
        _dev(x, inds2d, skip, W)
        x, skip = _f32c(x), _f32c(skip)
        ctx.rev = reverse_for(inds2d, first_column=True) if is_deterministic() else None
        inds2d, i64 = _idx(inds2d)
        Nq = inds2d.shape[0]
        if skip.shape[0] != Nq:
            raise RuntimeError("upsample_cat_linear: the skip features and the upsampling indices differ in length")
        stride = inds2d.shape[1] if inds2d.dim() == 2 else 1
        C1, C2 = x.shape[1], skip.shape[1]
        ctx.split_form = bool(DECODER_SPLIT and Nq > 0 and x.shape[0] > 0 and C1 > 0 and C2 > 0 and W.shape[0] > 0)
        if ctx.split_form:
            W = _f32c(W)
            if W.shape[1] != C1 + C2:
                raise RuntimeError("upsample_cat_linear: the weight has %d input columns, the inputs %d + %d" % (W.shape[1], C1, C2))
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(x, skip, W, inds2d)
            ctx.dims = (x.shape[0], C1, C2, stride, i64)
            Yc, _ = _nt_ldb_add(x, W, 0, C1)
            y, st = _nt_ldb_add(skip, W, C1, C2, (Yc, inds2d, i64, stride), stats_n_valid, finish)
            if st is not None:
                ctx.mark_non_differentiable(st.partials)
            return y, st
        cat = torch.empty((Nq, C1 + C2), device=x.device, dtype=torch.float32)
        check(lib().mvk_gather_rows_cat_fwd(_p(x), x.shape[0], C1, _p(inds2d), i64, Nq, stride, _p(skip), C2, _p(cat),
                                            _stream()))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(cat, W, inds2d)
        ctx.dims = (x.shape[0], C1, C2, stride, i64)
        y, st = _product(cat, W, transB=True, stats_n_valid=stats_n_valid, finish=finish)
        if st is not None:
            ctx.mark_non_differentiable(st.partials)
        return y, st

    @staticmethod
    def _backward_split(ctx, g):
        x, skip, W, inds2d = ctx.saved_tensors
        ns, C1, C2, stride, i64 = ctx.dims
        need_x, need_skip, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        g = _f32c(g)
        Nq, N = g.shape
        split_arena_prepare(g.device)
        det = False
        if is_deterministic():
            det = ctx.rev is not None and ctx.rev.shape[0] >= ns
            if not det:
                _no_reverse_list("a closest_pool / upsampling matrix")
        Gc = None
        if need_x or need_w:
            # G_c[j] = the sum of the gradient rows of coarse point j's fine points: a gather over the reverse list in a fixed
            # order, or the atomic row scatter (shadow indices dropped; coarse rows nobody points at stay zero)
            if det:
                Gc = gather_sum_rows(g, ctx.rev[:ns])
            else:
                Gc = _zeros((ns, N), g.device)
                check(lib().mvk_gather_rows_bwd_ld(_p(g), N, _p(inds2d), i64, Nq, stride, ns, N, _p(Gc), _stream()))
        dx = d_skip = None
        if need_x and need_skip and not det:
            plan = (C.c_int * 3)()
            check(lib().mvk_gemm_f32_nn_pair_plan(ns, C1, Nq, C2, N, plan))
            if plan[0]:
                dx = _split_out((ns, C1), g.device, plan[1])
                d_skip = _split_out((Nq, C2), g.device, plan[2])
                check(lib().mvk_gemm_f32_nn_pair(_p(Gc), _p(W), _p(dx), ns, C1, _p(g), C.c_void_p(W.data_ptr() + 4 * C1),
                                                 _p(d_skip), Nq, C2, N, C1 + C2, _stream()))
        if need_x and dx is None:
            dx = gemm_ldb(Gc, W, 0, C1, C1 + C2)
        if need_skip and d_skip is None:
            d_skip = gemm_ldb(g, W, C1, C2, C1 + C2)
        dW = _dw_gemm_slabs([(Gc, x), (g, skip)], target=W) if need_w else None
        return dx, None, d_skip, dW, None, None

    @staticmethod
    def backward(ctx, g, g_st=None):
        if g is None:                       # (set_materialize_grads(False): the output was not used)
            return None, None, None, None, None, None
        if ctx.split_form:
            return _UpsampleCatLinearFn._backward_split(ctx, g)
        cat, W, inds2d = ctx.saved_tensors
        ns, C1, C2, stride, i64 = ctx.dims
        g = _f32c(g)
        M, N, Kd = cat.shape[0], C1 + C2, W.shape[0]
        split_arena_prepare(g.device)
        if is_deterministic() and M > 0:
            rev = ctx.rev
            if rev is not None and rev.shape[0] >= ns:
                # (sum of the gradient rows of every coarse point's fine points) . W[:, :C1]: the scatter as a gather, then
                # the two halves of g W as two products -- fixed summation order throughout
                dx = gemm_ldb(gather_sum_rows(g, rev[:ns]), W, 0, C1, N) if ctx.needs_input_grad[0] else None
                d_skip = gemm_ldb(g, W, C1, C2, N) if ctx.needs_input_grad[2] else None
                dW = _dw_gemm(g, cat, target=W) if ctx.needs_input_grad[3] else None
                return dx, None, d_skip, dW, None, None
            _no_reverse_list("a closest_pool / upsampling matrix")
        dx = _zeros((ns, C1), g.device)
        split = gemm_plan(M, N, Kd, None, False)[0] if M > 0 else 1
        d_skip = _split_out((M, C2), g.device, split)
        if M > 0:
            check(lib().mvk_gemm_f32_scatter_cat(_p(g), _p(W), M, N, Kd, _p(inds2d), i64, stride, ns, C1, _p(dx),
                                                 _p(d_skip), _stream()))
        dW = _dw_gemm(g, cat, target=W) if ctx.needs_input_grad[3] else None
        return (dx if ctx.needs_input_grad[0] else None), None, (d_skip if ctx.needs_input_grad[2] else None), dW, None, None


def upsample_cat_linear(x, inds, skip, W, stats_n_valid=None, bn=None):
    """linear(upsample_cat(x, inds, skip), W, stats_n_valid=...) with a one-launch backward for x and skip."""
    y, st = _UpsampleCatLinearFn.apply(x, inds, skip, W, stats_n_valid,
                                       bn if stats_n_valid is not None and _finishable(bn) else None)
    if st is not None:
        y._mvk_bn_stats = st
    return y


def upsample_cat(x, inds, skip):
    """torch.cat([closest_pool(x, inds), skip], dim=1) of the KPFCNN decoder (blocks.py:79-91, architectures.py:334)."""
    return _UpsampleCatFn.apply(x, inds, skip)


def max_pool(x, inds, passthrough=False):
    """blocks.py:94-110 (zero shadow row takes part in the max). passthrough=True returns (pooled, x') with x' an alias
    of x for another consumer of x, whose gradient the backward accumulates onto (see linear())."""
    out, alias = _MaxPoolFn.apply(x, inds, passthrough)
    return (out, alias) if passthrough else out


def closest_pool(x, inds):
    """blocks.py:79-91 (first column = closest neighbour because rows are sorted)."""
    return _GatherRowsFn.apply(x, inds)


# --------------------------------------------------------------------------------------------
# input pyramid: grid subsampling + radius neighbours (device resident)
# --------------------------------------------------------------------------------------------

import numpy as _np

_WS = {}


def _workspace(tag, nbytes, device):
    """Grow-only HBM scratch per (tag, device); owned by the Python host layer, handed to the C ABI."""
    key = (tag, device.index)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _lens_host(lens):
    if isinstance(lens, torch.Tensor):
        lens = lens.detach().cpu().numpy()
    return _np.ascontiguousarray(lens, dtype=_np.int32)


def grid_subsample_batch(points, lens, features=None, labels=None, dl=0.1, max_p=0, rotations=None):
    """Device version of cpp_subsampling.subsample_batch (wrapper.cpp:62-333).

    points [N,3] f32 (HBM), lens host int32 [B], optional features [N,fdim] f32 and labels [N,ldim]
    int32 (HBM). Returns (s_points [M,3] HBM, s_lens np.int32 [B][, s_features][, s_labels]).
    Bit-identical to the reference incl. output order. Synchronises once (the counts come back to the host).
    rotations (host float32 [B,3,3]): the random grid orientation of batch_grid_subsampling
    (datasets/common.py:89-134) applied inside the same call (rotate, subsample, rotate back)."""
    _dev(points, features, labels)
    points = _f32c(points)
    lens_h = _lens_host(lens)
    N, B = points.shape[0], int(lens_h.shape[0])
    fdim = ldim = 0
    if features is not None:
        features = _f32c(features)
        fdim = features.shape[1]
    if labels is not None:
        labels = labels.to(torch.int32).contiguous()
        if labels.dim() == 1:
            labels = labels.unsqueeze(1)
        ldim = labels.shape[1]
    ws = _workspace("sub", lib().mvk_grid_subsample_workspace(N, B, fdim, ldim), points.device)
    out_pts = torch.empty((max(N, 1), 3), device=points.device, dtype=torch.float32)
    out_f = torch.empty((max(N, 1), fdim), device=points.device, dtype=torch.float32) if fdim else None
    out_l = torch.empty((max(N, 1), ldim), device=points.device, dtype=torch.int32) if ldim else None
    out_lens = torch.empty((B,), device=points.device, dtype=torch.int32)
    out_lens_h = _np.empty((B,), _np.int32)
    tail = (_p(features), fdim, _p(labels), ldim, float(dl), int(max_p), _p(out_pts), _p(out_f), _p(out_l),
            _p(out_lens), out_lens_h.ctypes.data_as(C.c_void_p), _p(ws), ws.numel(), _stream())
    if rotations is None:
        check(lib().mvk_grid_subsample_batch(_p(points), N, lens_h.ctypes.data_as(C.c_void_p), B, *tail))
    else:
        rot = _np.ascontiguousarray(rotations, dtype=_np.float32)
        if rot.shape != (B, 3, 3):
            raise RuntimeError("grid_subsample_batch: rotations must be [B,3,3]")
        check(lib().mvk_grid_subsample_batch_oriented(_p(points), N, lens_h.ctypes.data_as(C.c_void_p), B,
                                                      rot.ctypes.data_as(C.c_void_p), *tail))
    M = int(out_lens_h.sum())
    res = [out_pts[:M], out_lens_h]
    if fdim:
        res.append(out_f[:M])
    if ldim:
        res.append(out_l[:M])
    return tuple(res)


_NB_GRID = {}      # device index -> workspace address that holds the last built grid


def radius_neighbors_batch(queries, supports, q_lens, s_lens, radius, limit=None, status=None, reuse_grid=False):
    """Device version of cpp_neighbors.batch_query (wrapper.cpp:58-238): int32 [Nq, W] in HBM.

    limit=None: W = the data-dependent max count (one extra counting pass + host sync, like the
    reference's two-pass fill); limit=k: keep the k nearest per row (= big_neighborhood_filter,
    datasets/common.py:411-421) without the counting pass, W = min(k, max count) like the reference.

    status (int32 [2] HBM tensor, needs limit): enqueue-only mode for a sync-free pyramid -- W = limit
    always, nothing is read back; status accumulates [max row count, overflow flag] for ONE later check
    (check_neighbor_status). reuse_grid=True (enqueue-only mode): the caller guarantees that the previous
    search on this device used the same supports, s_lens and radius, so its cell grid is reused."""
    _dev(queries, supports)
    q, s = _f32c(queries), _f32c(supports)
    ql, sl = _lens_host(q_lens), _lens_host(s_lens)
    if ql.shape[0] != sl.shape[0]:
        raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
    Nq, Ns, B = q.shape[0], s.shape[0], int(ql.shape[0])
    ws = _workspace("nb", lib().mvk_radius_neighbors_workspace(Nq, Ns, B), q.device)
    args = (_p(q), Nq, _p(s), Ns, ql.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p), B, float(radius))
    if status is not None:
        if limit is None:
            raise RuntimeError("radius_neighbors_batch: the enqueue-only mode needs a column limit")
        _dev(status)
        width = int(limit)
        out = torch.empty((Nq, width), device=q.device, dtype=torch.int32)
        reuse = bool(reuse_grid) and _NB_GRID.get(q.device.index) == ws.data_ptr()   # a regrown workspace lost the grid
        if width > 0 and Nq > 0:
            check(lib().mvk_radius_neighbors_enqueue(*args, _p(out), width, _p(status), int(reuse), _p(ws),
                                                     ws.numel(), _stream()))
            _NB_GRID[q.device.index] = ws.data_ptr()
        return out
    _NB_GRID.pop(q.device.index, None)
    if limit is None:
        w = C.c_int(0)
        check(lib().mvk_radius_neighbors_batch(*args, None, 0, C.byref(w), _p(ws), ws.numel(), _stream()))
        width = int(w.value)
    else:
        width = int(limit)
    out = torch.empty((Nq, width), device=q.device, dtype=torch.int32)
    if width > 0 and Nq > 0:
        w = C.c_int(0)
        check(lib().mvk_radius_neighbors_batch(*args, _p(out), width, C.byref(w), _p(ws), ws.numel(), _stream()))
        if int(w.value) < width:            # reference shape: min(limit, data-dependent max count)
            out = out[:, :int(w.value)].contiguous()
    return out


def grid_subsample_dev(points, lens_dev, dl, out_points, out_lens_dev, status, rotations_dev=None,
                       total_out=None, pad_value=1e6):
    """Capturable subsampling (mvk_grid_subsample_batch_dev): points [cap_in,3] with DEVICE lens [B] ->
    out_points [out_cap,3] (rows past the total = pad_value), out_lens_dev [B], total_out [1]. No host sync."""
    _dev(points, lens_dev, out_points, out_lens_dev, status, rotations_dev, total_out)
    points = _f32c(points)
    cap_in, B = points.shape[0], int(lens_dev.shape[0])
    if not out_points.is_contiguous() or out_points.dtype != torch.float32:
        raise RuntimeError("grid_subsample_dev: out_points must be a contiguous float32 [cap,3] tensor")
    ws = _workspace("sub", lib().mvk_grid_subsample_workspace(cap_in, B, 0, 0), points.device)
    check(lib().mvk_grid_subsample_batch_dev(_p(points), cap_in, _p(lens_dev), B, _p(rotations_dev), float(dl),
                                             _p(out_points), out_points.shape[0], float(pad_value),
                                             _p(out_lens_dev), _p(total_out), _p(status), _p(ws), ws.numel(), _stream()))


def radius_neighbors_dev(queries, supports, q_lens_dev, s_lens_dev, radius, out, shadow, status, reuse_grid=False,
                         rev=None, rev_counts=None, rev_status=None):
    """Capturable neighbour search (mvk_radius_neighbors_dev) into the fixed matrix out [Nq_cap, width] int32.
    rev [Ns_cap, Hr] int32 + rev_counts [Ns_cap] int32 (zero) + rev_status [2]: the search also fills the transposed
    relation while it writes the rows (mvk_radius_neighbors_dev_rev, width <= 64; rows in order of arrival); finish the
    lists of the whole pyramid with reverse_finish_many()."""
    _dev(queries, supports, q_lens_dev, s_lens_dev, out, status, rev, rev_counts, rev_status)
    q, s = _f32c(queries), _f32c(supports)
    if out.dtype != torch.int32 or not out.is_contiguous() or out.shape[0] != q.shape[0]:
        raise RuntimeError("radius_neighbors_dev: out must be a contiguous int32 [Nq_cap, width] tensor")
    B = int(q_lens_dev.shape[0])
    ws = _workspace("nb", lib().mvk_radius_neighbors_workspace(q.shape[0], s.shape[0], B), q.device)
    if rev is not None:
        if (rev.dtype != torch.int32 or not rev.is_contiguous() or rev.dim() != 2 or rev.shape[0] < s.shape[0]
                or rev_counts is None or rev_counts.dtype != torch.int32 or rev_counts.numel() < s.shape[0] or rev_status is None):
            raise RuntimeError("radius_neighbors_dev: rev must be a contiguous int32 [>= Ns_cap, Hr] matrix with int32 "
                               "counters [>= Ns_cap] and a status word")
        check(lib().mvk_radius_neighbors_dev_rev(_p(q), q.shape[0], _p(s), s.shape[0], _p(q_lens_dev), _p(s_lens_dev), B,
                                                 float(radius), _p(out), out.shape[1], int(shadow), _p(status),
                                                 int(bool(reuse_grid)), _p(ws), ws.numel(), _p(rev), rev.shape[1],
                                                 _p(rev_counts), _p(rev_status), _stream()))
    else:
        check(lib().mvk_radius_neighbors_dev(_p(q), q.shape[0], _p(s), s.shape[0], _p(q_lens_dev), _p(s_lens_dev), B,
                                             float(radius), _p(out), out.shape[1], int(shadow), _p(status),
                                             int(bool(reuse_grid)), _p(ws), ws.numel(), _stream()))
    _NB_GRID.pop(q.device.index, None)


REG_MANY = CONSTANTS["MVK_REG_MANY"]
REV_MANY = CONSTANTS["MVK_REV_MANY"]


def reverse_finish_many(lists, status=None):
    """lists: [(rev [rows, Hr] int32, counts [>= rows] int32, rows, shadow)] filled by radius_neighbors_dev(rev=...): pads the
    tails, returns the counters to zero and accumulates the longest row into status[0] -- one launch for up to 12 lists
    (mvk_reverse_finish_many)."""
    from ._lib import RevList
    for i0 in range(0, len(lists), REV_MANY):
        chunk = lists[i0:i0 + REV_MANY]
        arr = (RevList * len(chunk))()
        for k, (rev, counts, rows, shadow) in enumerate(chunk):
            _dev(rev, counts, status)
            arr[k] = RevList(_p(rev), _p(counts), _p(status), int(rows), int(rev.shape[1]), int(shadow))
        check(lib().mvk_reverse_finish_many(arr, len(chunk), _stream()))


def neighbors_cell_order(Nq, Ns, B, out=None, s_lens_dev=None, device=None):
    """Work list for kpconv(order=...) out of the cell grid the LAST neighbour search on this device built
    (mvk_neighbors_cell_order; the search must have had these Nq / Ns / B -- the capacities for radius_neighbors_dev,
    whose device lengths go in s_lens_dev): the support rows sorted by cloud, grid cell and row, int32 [Ns] (or written
    into `out` [cap >= Ns], identity beyond the clouds' rows). One launch, no synchronisation."""
    dev = out.device if out is not None else (s_lens_dev.device if s_lens_dev is not None else device)
    if out is None:
        out = torch.empty((Ns,), device=dev, dtype=torch.int32)
    _dev(out, s_lens_dev)
    if out.dtype != torch.int32 or not out.is_contiguous() or out.dim() != 1 or out.shape[0] < Ns:
        raise RuntimeError("neighbors_cell_order: out must be a contiguous int32 vector of at least Ns entries")
    ws = _workspace("nb", lib().mvk_radius_neighbors_workspace(Nq, Ns, B), dev)
    check(lib().mvk_neighbors_cell_order(Ns, B, _p(s_lens_dev), _p(out), out.shape[0], _p(ws), ws.numel(), _stream()))
    return out


_REV_COUNTS = {}      # device index -> persistent zero int32 buffer of mvk_reverse_neighbors (self-cleaning)
_REV_COUNTS_RETIRED = []      # outgrown buffers: a graph captured earlier still adds into and zeroes its old address
REVERSE_DX = os.environ.get("MVK_REVERSE_DX", "1") == "1"      # development switch: 0 = the scatter backward everywhere


def _rev_counts(n, device):
    # one buffer per device: reverse lists are built by ONE stream at a time (the input side of a step); two builds
    # running concurrently on different streams would share the counters
    key = device.index
    buf = _REV_COUNTS.get(key)
    if buf is None or buf.numel() < n:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ops.reverse_neighbors: the counter buffer of this device does not exist yet (or is too "
                               "small) and cannot be created inside a graph capture; build one batch eagerly first")
        if buf is not None:
            # never handed back to the allocator: replays of earlier captures keep using it
            _REV_COUNTS_RETIRED.append(buf)
        buf = torch.zeros(max(int(n), 1 << 16), dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()      # zero before any other stream's build uses it
        _REV_COUNTS[key] = buf
    return buf


REV_MAX_WIDTH = CONSTANTS["MVK_REV_MAX_WIDTH"]


def reverse_width_cap(sort=None):
    """Longest row a reverse list may have (8192, sorted or not): the wide relations of the deformable layers -- a support
    near the middle of a coarse level is a neighbour of almost every query at the deform radius."""
    return REV_MAX_WIDTH


def reverse_neighbors(idx, Ns, width=None, out=None, status=None, shadow=None, sort=None, first_column=False):
    """The transposed neighbourhood relation of idx [Nq, H] (int32 / int64, entries outside [0, Ns) = shadow): rev
    [Ns, width] int32, row j = the rows n of idx that contain j, padded with `shadow` (default Nq)
    (mvk_reverse_neighbors). It turns the feature gradient of a rigid KPConv into a gather (kpconv(..., rev=...)).
    sort: rows ascending (what run-to-run identical sums need; default: in deterministic mode) or in order of arrival
    (saves the ranking pass). first_column: the relation of idx[:, 0] alone (nearest upsampling).
    width None: the exact longest row (one read-back: eager use); with a width, `status` (int32 [2] HBM) accumulates
    [longest row, overflow] without any synchronisation -- check it with check_reverse_status. out: write into this
    int32 [>= Ns, width] matrix instead of allocating (capacity-padded batches)."""
    _dev(idx, out, status)
    idx, i64 = _idx(idx)
    Nq, H = idx.shape[0], idx.shape[1] if idx.dim() == 2 else 0
    stride = H
    if first_column:
        H = min(H, 1)
    Ns = int(Ns)
    shadow = Nq if shadow is None else int(shadow)
    dev = idx.device
    counts = _rev_counts(Ns, dev)
    do_sort = int(is_deterministic() if sort is None else bool(sort))

    def run(dst, w, st):
        check(lib().mvk_reverse_neighbors(_p(idx), i64, Nq, H, max(stride, H), Ns, _p(dst), int(w), shadow, do_sort,
                                          _p(counts), _p(st), _stream()))

    if out is not None:
        if out.dtype != torch.int32 or not out.is_contiguous() or out.dim() != 2 or out.shape[0] < Ns:
            raise RuntimeError("reverse_neighbors: out must be a contiguous int32 [>= Ns, width] matrix")
        run(out, out.shape[1], status)
        return out
    if width is not None:
        rev = torch.empty((Ns, max(int(width), 1)), device=dev, dtype=torch.int32)
        run(rev, rev.shape[1], status)
        return rev
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    cap = reverse_width_cap(do_sort)
    w = max(8, min(cap, 2 * H + 8))
    rev = torch.empty((Ns, w), device=dev, dtype=torch.int32)
    run(rev, w, st)
    longest, ovf = (int(v) for v in st.cpu())
    if ovf:
        if longest > cap:
            raise RuntimeError("reverse_neighbors: a support has %d reverse neighbours (> %d)" % (longest, cap))
        rev = torch.empty((Ns, longest), device=dev, dtype=torch.int32)
        run(rev, longest, None)
        return rev
    return rev[:, :max(longest, 1)].contiguous()


# reverse lists of pooling / upsampling matrices, found again by the matrix itself (the blocks hand max_pool and
# closest_pool nothing but `batch.pools[l]` / `batch.upsamples[l]`): deterministic mode's gather-form backwards
_REVERSES = collections.OrderedDict()
_REVERSES_KEPT = 256


def _rev_key(inds, first):
    return (inds.device.index, inds.data_ptr(), tuple(inds.shape), inds.dtype, bool(first))


def remember_reverse(inds, rev, first_column=False):
    """Registers rev = reverse_neighbors(inds, ...) (first_column: of inds[:, 0]) under the index matrix itself. The
    entry holds a weak reference to THAT tensor object: another matrix of the same shape at a recycled address never
    matches (a wrong reverse list would be a silently wrong gradient, unlike a stale work list)."""
    key = _rev_key(inds, first_column)
    if len(_REVERSES) >= 16:
        # entries whose index matrix is gone hold tens of MB each at level 0: drop them now, not 256 batches later
        for k in [k for k, e in _REVERSES.items() if e[0]() is None]:
            del _REVERSES[k]
    _REVERSES[key] = (weakref.ref(inds), rev)
    _REVERSES.move_to_end(key)
    while len(_REVERSES) > _REVERSES_KEPT:
        _REVERSES.popitem(last=False)


def reverse_for(inds, first_column=False):
    """The reverse list registered for this very tensor object (call it where the matrix is still the object the batch
    holds: in the forward), or None."""
    if not (torch.is_tensor(inds) and inds.is_cuda):
        return None
    e = _REVERSES.get(_rev_key(inds, first_column))
    return e[1] if (e is not None and e[0]() is inds) else None


_DET_WARNED = set()


def _no_reverse_list(what):
    """Deterministic mode met a scatter without a reverse list (a deformable block's pooling, a batch that was moved
    or rebuilt outside datasets.common): the atomic path runs, the result is correct but not bit-reproducible."""
    if what not in _DET_WARNED:
        _DET_WARNED.add(what)
        import warnings
        warnings.warn("deterministic mode: no reverse list for %s; its backward uses float atomics (not bit-reproducible)" % what)


def gather_sum_rows(g, rev, base=None):
    """out[j] = (base[j] or 0) + sum of g[n] over the entries n of rev[j] (mvk_gather_sum_rows); g [Nq, C] may be a column
    block of a wider tensor (row stride >= C)."""
    _dev(g, rev, base)
    if not (g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1 and g.stride(0) >= g.shape[1]):
        g = _f32c(g)
    Ns, Hr = rev.shape
    out = torch.empty((Ns, g.shape[1]), device=g.device, dtype=torch.float32)
    if base is not None:
        base = _f32c(base)
    check(lib().mvk_gather_sum_rows(_p(g), g.stride(0), g.shape[0], _p(rev), Hr, Ns, g.shape[1], _p(base), _p(out), _stream()))
    return out


def gemm_ldb(A, B_base, col0, N, ldb):
    """A [M,Kd] @ B[:, col0:col0+N] for a row-major B [Kd, ldb] read in place (mvk_gemm_f32_ldb)."""
    _dev(A, B_base)
    A, B_base = _f32c(A), _f32c(B_base)
    M, Kd = A.shape
    split_arena_prepare(A.device)
    out = _split_out((M, N), A.device, gemm_plan(M, N, Kd)[0] if M > 0 and N > 0 else 1)
    if M > 0 and N > 0:
        check(lib().mvk_gemm_f32_ldb(_p(A), C.c_void_p(B_base.data_ptr() + 4 * int(col0)), _p(out), M, int(N), Kd, int(ldb),
                                     _stream()))
    return out


def check_reverse_status(status):
    """Reads a reverse-list status word back (synchronises): raises when a row did not fit its width."""
    longest, ovf = (int(v) for v in status.cpu())
    if ovf:
        raise RuntimeError("reverse neighbours: a support row has %d entries, more than the width it was built with"
                           % longest)
    return longest


def _neg_kernel_points(kp):
    """-kp, cached on the tensor (kernel points are frozen parameters; the cache follows in-place updates)."""
    c = getattr(kp, "_mvk_neg", None)
    if c is None or c[0] != kp._version:
        c = (kp._version, (-kp.detach()).contiguous())
        kp._mvk_neg = c
    return c[1]


def kp_transposed_contraction(A2, W):
    """dx [M, Cin] = sum_k A2[:, k, :] . W[k]^T for A2 [M, K, Cout], W [K, Cin, Cout] (mvk_gemm_f32_kp_transposed; a Cout
    that is not a power of two >= 32 -- the 45 / 60 offset channels of a deformable layer's inner convolution -- takes a
    transposed copy of the weights and the plain product)."""
    _dev(A2, W)
    A2, W = _f32c(A2), _f32c(W)
    M, K, Cout = A2.shape
    Cin = W.shape[1]
    if W.shape[0] != K or W.shape[2] != Cout:
        raise RuntimeError("kp_transposed_contraction: A2 [M,K,Cout] and W [K,Cin,Cout] expected")
    if Cout < 32 or (Cout & (Cout - 1)) != 0:
        return gemm(A2.view(M, K * Cout), W.permute(0, 2, 1).reshape(K * Cout, Cin).contiguous())
    split_arena_prepare(A2.device)
    split = gemm_plan(M, Cin, K * Cout)[0] if M > 0 else 1
    dx = _split_out((M, Cin), A2.device, split)
    if M > 0:
        check(lib().mvk_gemm_f32_kp_transposed(_p(A2), _p(W), _p(dx), M, K, Cin, Cout, _stream()))
    return dx


_WORK_ORDERS = collections.OrderedDict()      # (device index, address, rows) of a points tensor -> its work list
_WORK_ORDERS_KEPT = 64


def remember_work_order(points, order):
    """Side channel for batch containers that cannot carry the lists (the reference's flat input_list): the work list
    of a level, found again by the address and row count of its points tensor. A stale hit (another cloud of the same
    size at a recycled address) is still a permutation of its rows, which is all the gather needs."""
    key = (points.device.index, points.data_ptr(), points.shape[0])
    _WORK_ORDERS[key] = order
    _WORK_ORDERS.move_to_end(key)
    while len(_WORK_ORDERS) > _WORK_ORDERS_KEPT:
        _WORK_ORDERS.popitem(last=False)


def work_order_for(points):
    return _WORK_ORDERS.get((points.device.index, points.data_ptr(), points.shape[0])) if points.is_cuda else None


def check_neighbor_status(status):
    """Reads an enqueue-only status word back (synchronises with the work that produced it)."""
    maxc, ovf = (int(v) for v in status.cpu())
    if ovf:
        raise RuntimeError("neighbors: a query has more in-range supports than the in-kernel list holds")
    return maxc


def pad_points(src, dst, fill, count_out=None):
    """dst [cap,w] <- src [n,w] padded with `fill`; count_out (int32 [1] HBM) <- n. One launch."""
    _dev(src, dst, count_out)
    src = _f32c(src)
    if not dst.is_contiguous() or dst.dtype != torch.float32 or dst.shape[1] != src.shape[1]:
        raise RuntimeError("pad_points: destination must be a contiguous float32 [cap, %d] tensor" % src.shape[1])
    check(lib().mvk_pad_points(_p(src), src.shape[0], _p(dst), dst.shape[0], src.shape[1], float(fill),
                               _p(count_out), _stream()))


def pad_index_rows(src, shadow_src, dst, shadow_dst):
    """dst [cap,w_dst] <- src [n,w_src] with the shadow index rewritten, padded with shadow_dst. One launch."""
    _dev(src, dst)
    src, i64 = _idx(src)
    if dst.dtype != src.dtype or not dst.is_contiguous():
        raise RuntimeError("pad_index_rows: destination must be contiguous and of the source's index type")
    w_src = src.shape[1] if src.dim() == 2 else 0
    check(lib().mvk_pad_index_rows(_p(src), i64, src.shape[0], w_src, int(shadow_src), _p(dst), dst.shape[0],
                                   dst.shape[1], int(shadow_dst), _stream()))


# --------------------------------------------------------------------------------------------
# 2D -> 3D fusion
# --------------------------------------------------------------------------------------------

def unproject_depth(depth_mm, cam_matrix, poses):
    """depth (nv,h,w) uint16/int16-compatible HBM tensor [mm], cam_matrix (>=3x3) float32 host array
    (already rescaled to the image size), poses (nv,4,4) f32 HBM -> (xyz (nv,h,w,3) f64, valid (nv,h,w) bool).
    ScanNet_sphere_color.py:66-72,409-417 (float64 because the pixel grid is int64 there)."""
    _dev(depth_mm, poses)
    nv, h, w = depth_mm.shape
    d16 = depth_mm.to(torch.int16).contiguous() if depth_mm.dtype != torch.int16 else depth_mm.contiguous()
    kinv = _np.linalg.inv(_np.asarray(cam_matrix, dtype=_np.float32)[:3, :3]).astype(_np.float64)  # :71 (f32 inverse)
    kinv = _np.ascontiguousarray(kinv)
    poses = _f32c(poses)
    xyz = torch.empty((nv, h, w, 3), device=depth_mm.device, dtype=torch.float64)
    valid = torch.empty((nv, h, w), device=depth_mm.device, dtype=torch.uint8)
    check(lib().mvk_unproject_depth(_p(d16), nv, h, w, kinv.ctypes.data_as(C.c_void_p), _p(poses), _p(xyz),
                                    _p(valid), _stream()))
    return xyz, valid.bool()


def knn_pixels(sphere_points, image_xyz, image_mask, k=3):
    """Exact k-NN (float64) of sphere points among valid unprojected pixels -> flat pixel indices
    view*h*w + row*w + col, int64 [ns,k] (ScanNet_sphere_color.py:436-451)."""
    _dev(sphere_points, image_xyz, image_mask)
    q = _f32c(sphere_points)
    keys = image_xyz.reshape(-1, 3).to(torch.float64).contiguous()
    valid = image_mask.reshape(-1).to(torch.uint8).contiguous()
    nq, nk = q.shape[0], keys.shape[0]
    ws = _workspace("knn", lib().mvk_knn_workspace(nq, nk, k), q.device)
    out = torch.empty((nq, k), device=q.device, dtype=torch.int64)
    check(lib().mvk_knn_f64(_p(q), nq, _p(keys), _p(valid), nk, int(k), _p(out), _p(ws), ws.numel(), _stream()))
    return out


# --------------------------------------------------------------------------------------------
# transposed index of the PointNet++ ops (csrc/pn2_ordered.hip): deterministic mode's gather-form backwards
# --------------------------------------------------------------------------------------------

def index_csr(index, n1, status=None):
    """The transposed index of group_points / feature_interpolate (mvk_index_csr): index (B,N2,K) or (B,L) int64 in HBM
    with keys in [0, n1) -> (row_start, entries), both int32: row (b, j) = entries[row_start[b*n1 + j] :
    row_start[b*n1 + j + 1]] = the flat positions p = n*K + k of batch element b that hold key j, ascending. Entries
    outside [0, n1) are in no row; `status` (int32 word in HBM, e.g. pn2_index_status(device)) is set to 1 when one is
    met. No synchronisation, nothing read back; the scratch is this call's own, so the call can be captured in a graph
    and two builds may run on two streams."""
    _dev(index, status)
    if index.dtype != torch.int64 or index.dim() not in (2, 3):
        raise RuntimeError("index_csr: expected an int64 index (B,N2,K) or (B,L)")
    index = index.contiguous()
    B, n1 = index.shape[0], int(n1)
    L = index.numel() // B if B > 0 else 0
    if n1 < 0 or B * L >= 1 << 31 or B * n1 >= 1 << 31:
        raise RuntimeError("index_csr: B*L = %d and B*n1 = %d must be below 2^31" % (B * L, B * n1))
    row_start = torch.empty((B * n1 + 1,), device=index.device, dtype=torch.int32)
    entries = torch.empty((B * L,), device=index.device, dtype=torch.int32)
    nbytes = lib().mvk_index_csr_workspace(B, L, n1)
    ws = torch.empty((max(nbytes, 4),), device=index.device, dtype=torch.uint8)
    check(lib().mvk_index_csr(_p(index), B, L, n1, _p(row_start), _p(entries), _p(status), _p(ws), ws.numel(), _stream()))
    return row_start, entries


_INDEX_CSRS = collections.OrderedDict()
_INDEX_CSRS_KEPT = 64


def _csr_key(index, n1):
    return (index.device.index, index.data_ptr(), tuple(index.shape), int(n1))


def remember_index_csr(index, n1, csr):
    """Registers csr = index_csr(index, n1) under the index tensor itself, like remember_reverse: the entry holds a weak
    reference to THAT tensor object and its version counter, so neither another tensor at a recycled address nor the same
    tensor after an in-place write ever matches."""
    for k in [k for k, e in _INDEX_CSRS.items() if e[0]() is None]:
        del _INDEX_CSRS[k]
    key = _csr_key(index, n1)
    _INDEX_CSRS[key] = (weakref.ref(index), index._version, csr)
    _INDEX_CSRS.move_to_end(key)
    while len(_INDEX_CSRS) > _INDEX_CSRS_KEPT:
        _INDEX_CSRS.popitem(last=False)


def index_csr_for(index, n1):
    """The (row_start, entries) registered for this very tensor object and key count, or None."""
    if not (torch.is_tensor(index) and index.is_cuda):
        return None
    e = _INDEX_CSRS.get(_csr_key(index, n1))
    return e[2] if (e is not None and e[0]() is index and e[1] == index._version) else None


def _index_csr_shared(owner, index, n1):
    """The CSR of `index` (the contiguous form of the caller's tensor `owner`), built once per owner."""
    csr = index_csr_for(owner, n1)
    if csr is None:
        csr = index_csr(index, n1)
        remember_index_csr(owner, n1, csr)
    return csr


class _GroupPointsFn(torch.autograd.Function):
    """mvpnet/ops/group_points.py:5-17; float32 and float64 like the reference's extension."""

    @staticmethod
    def forward(ctx, points, index):
        _dev(points, index)
        if index.dtype != torch.int64:
            raise RuntimeError("group_points: index must be int64")
        if points.dim() != 3 or index.dim() != 3 or points.shape[0] != index.shape[0]:
            raise RuntimeError("group_points: expected points (B,C,N1) and index (B,N2,K)")
        f64 = points.dtype == torch.float64
        caller_index = index
        points, index = (points.contiguous() if f64 else _f32c(points)), index.contiguous()
        B, Cc, N1 = points.shape
        _, N2, K = index.shape
        out = torch.empty((B, Cc, N2, K), device=points.device, dtype=points.dtype)
        fn = lib().mvk_group_points_fwd_f64 if f64 else lib().mvk_group_points_fwd
        check(fn(_p(points), _p(index), B, Cc, N1, N2, K, _p(out), _stream()))
        ctx.save_for_backward(index)
        ctx.n1, ctx.f64 = N1, f64
        # deterministic mode: the backward is a gather over the transposed index, kept under the CALLER's tensor object
        # (QueryGrouper groups coordinates and features with one index: one CSR)
        ctx.det, ctx.csr_owner = is_deterministic(), caller_index
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (index,) = ctx.saved_tensors
        g = grad_out.double().contiguous() if ctx.f64 else _f32c(grad_out)
        B, Cc, N2, K = g.shape
        if ctx.det:
            row_start, entries = _index_csr_shared(ctx.csr_owner, index, ctx.n1)
            gi = torch.empty((B, Cc, ctx.n1), device=g.device, dtype=g.dtype)       # every element is written
            fn = lib().mvk_group_points_bwd_csr_f64 if ctx.f64 else lib().mvk_group_points_bwd_csr
            check(fn(_p(g), _p(row_start), _p(entries), B, Cc, ctx.n1, N2, K, _p(gi), _stream()))
            return gi, None
        gi = torch.zeros((B, Cc, ctx.n1), device=g.device, dtype=g.dtype)
        fn = lib().mvk_group_points_bwd_f64 if ctx.f64 else lib().mvk_group_points_bwd
        check(fn(_p(g), _p(index), B, Cc, ctx.n1, N2, K, _p(gi), _stream()))
        return gi, None


def group_points(points, index):
    """points (B,C,N1), index (B,N2,K) int64 -> (B,C,N2,K) (mvpnet/ops/group_points.py:20-31)."""
    return _GroupPointsFn.apply(points, index)


# --------------------------------------------------------------------------------------------
# MVPNet baseline: the PointNet++ point ops (csrc/pn2.hip), float32 and float64
# --------------------------------------------------------------------------------------------

def _pn2_float(name, *ts):
    """Contiguous detached operands of one floating dtype (the reference dispatches float and double)."""
    _dev(*ts)
    dt = ts[0].dtype
    if dt not in (torch.float32, torch.float64) or any(t.dtype != dt for t in ts):
        raise RuntimeError("%s: operands must all be float32 or all be float64" % name)
    return [t.detach().contiguous() for t in ts], dt == torch.float64


def _pn2_lengths(name, lengths, points):
    """The per-cloud point counts of a ragged point op: an int64 tensor (B,) on the device of `points` (B,N,D). Anything
    else is refused; the value and its form are checked before the device."""
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int64:
        raise RuntimeError("%s: lengths must be an int64 tensor, got %s"
                           % (name, lengths.dtype if isinstance(lengths, torch.Tensor) else type(lengths).__name__))
    if lengths.dim() != 1 or lengths.shape[0] != points.shape[0]:
        raise RuntimeError("%s: lengths must have shape (%d,), one count per cloud, got %s"
                           % (name, points.shape[0], tuple(lengths.shape)))
    _dev(lengths)
    if lengths.device != points.device:
        raise RuntimeError("%s: lengths on %s, points on %s" % (name, lengths.device, points.device))
    return lengths.detach().contiguous()


def fps(points, num_centroids, lengths=None):
    """Farthest point sampling: points (B,N,D) with D in {2,3} -> int64 (B,num_centroids), the reference's picks
    including its order among ties (mvpnet/ops/cuda/fps_kernel.cu:60-135). lengths: int64 (B,) on the points' device,
    for a padded batch: cloud b is points[b, :lengths[b]] (clamped to [1, N]), the rows behind it are never read, and
    row b of the result is what fps(points[b:b+1, :lengths[b]]) returns, the last pick repeated where num_centroids
    exceeds lengths[b] and no point is left at a positive distance."""
    if points.dim() != 3:
        raise RuntimeError("fps: expected points (B,N,D)")
    if lengths is not None:
        lengths = _pn2_lengths("fps", lengths, points)
    (pts,), f64 = _pn2_float("fps", points)
    B, N, D = pts.shape
    M = int(num_centroids)
    out = torch.empty((B, M if M > 0 else 0), device=pts.device, dtype=torch.int64)
    nbytes = lib().mvk_fps_workspace(B, N, int(f64))
    ws = torch.empty((nbytes,), device=pts.device, dtype=torch.uint8) if nbytes > 0 else None
    if lengths is not None:
        fn = lib().mvk_fps_ragged_f64 if f64 else lib().mvk_fps_ragged
        check(fn(_p(pts), _p(lengths), B, N, D, M, _p(out), _p(ws), nbytes, _stream()))
        return out
    fn = lib().mvk_fps_f64 if f64 else lib().mvk_fps
    check(fn(_p(pts), B, N, D, M, _p(out), _p(ws), nbytes, _stream()))
    return out


def pn2_ball_query(query, key, radius, max_neighbors, with_distance=False, key_lengths=None):
    """query (B,N1,3), key (B,N2,3) -> int64 (B,N1,K): the first K keys in index order with d2 < radius^2, padded with
    the first hit, -1 where there is none (ball_query_kernel.cu:59-135). with_distance: also d2 (B,N1,K), -1 in padded
    slots (ball_query_distance_kernel.cu). key_lengths: int64 (B,) on the keys' device, for a padded batch: the keys of
    batch element b are key[b, :key_lengths[b]] (clamped to [1, N2]); every query is answered."""
    if query.dim() != 3 or key.dim() != 3 or query.shape[2] != 3 or key.shape[2] != 3 \
            or query.shape[0] != key.shape[0]:
        raise RuntimeError("pn2_ball_query: expected query (B,N1,3) and key (B,N2,3)")
    if key_lengths is not None:
        key_lengths = _pn2_lengths("pn2_ball_query", key_lengths, key)
    (q, k), f64 = _pn2_float("pn2_ball_query", query, key)
    B, N1, _ = q.shape
    N2, K = k.shape[1], int(max_neighbors)
    index = torch.empty((B, N1, max(K, 0)), device=q.device, dtype=torch.int64)
    dist = torch.empty((B, N1, max(K, 0)), device=q.device, dtype=q.dtype) if with_distance else None
    if key_lengths is not None:
        fn = lib().mvk_pn2_ball_query_ragged_f64 if f64 else lib().mvk_pn2_ball_query_ragged
        check(fn(_p(q), _p(k), _p(key_lengths), B, N1, N2, float(radius), K, _p(index), _p(dist), _stream()))
        return (index, dist) if with_distance else index
    fn = lib().mvk_pn2_ball_query_f64 if f64 else lib().mvk_pn2_ball_query
    check(fn(_p(q), _p(k), B, N1, N2, float(radius), K, _p(index), _p(dist), _stream()))
    return (index, dist) if with_distance else index


def knn_distance(query, key, k=3):
    """query (B,N1,3), key (B,N2,3) -> int64 index (B,N1,3) and SQUARED distance (B,N1,3) in the input dtype, ascending,
    ties to the lower key index (knn_distance_kernel.cu:35-124). Only k = 3, like the reference."""
    (q, ky), f64 = _pn2_float("knn_distance", query, key)
    if q.dim() != 3 or ky.dim() != 3 or q.shape[2] != 3 or ky.shape[2] != 3 or q.shape[0] != ky.shape[0]:
        raise RuntimeError("knn_distance: expected query (B,N1,3) and key (B,N2,3)")
    B, N1, _ = q.shape
    N2 = ky.shape[1]
    index = torch.empty((B, N1, 3), device=q.device, dtype=torch.int64)
    dist = torch.empty((B, N1, 3), device=q.device, dtype=q.dtype)
    fn = lib().mvk_knn_distance_f64 if f64 else lib().mvk_knn_distance
    check(fn(_p(q), _p(ky), B, N1, N2, int(k), _p(index), _p(dist), _stream()))
    return index, dist


_PN2_STATUS = {}
_PN2_EAGER_CHECK = [os.environ.get("MVK_PN2_CHECK", "0") == "1"]


def pn2_index_status(device):
    """The int32 status word (on `device`) that the interpolation kernels set to 1 when they meet an index outside the
    key set (such an index contributes nothing). One word per device, allocated on first use."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _PN2_STATUS:
        _PN2_STATUS[key] = torch.zeros((1,), device=device, dtype=torch.int32)
    return _PN2_STATUS[key]


def pn2_check_indices(device=None):
    """Read the status word back (this waits for the device), clear it, and raise when an interpolation since the last
    check met an index outside its key set. Call it where a wait is affordable (end of an epoch, a test); with
    set_pn2_index_check(True) or MVK_PN2_CHECK=1 every feature_interpolate forward calls it itself."""
    status = pn2_index_status(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    bad = int(status.item())
    status.zero_()
    if bad:
        raise RuntimeError("feature_interpolate: an index lies outside the key set [0, N1)")


def set_pn2_index_check(flag):
    """True: every feature_interpolate forward waits for its status word and raises at once (one device-to-host read per
    call, not capturable in a graph). False (default): the word is only set; pn2_check_indices() reads it."""
    _PN2_EAGER_CHECK[0] = bool(flag)


class _FeatureInterpolateFn(torch.autograd.Function):
    """mvpnet/ops/interpolate.py:5-20. The backward is a float-atomic scatter-add by default; when set_deterministic was
    on in the forward it is the ordered gather over the transposed index (mvk_interpolate_bwd_csr). That CSR is built in
    the backward every time and not looked up: the build is what reports an index outside the key set, and the 3-NN
    index of a FeaturePropagation is a new tensor on every forward anyway."""

    @staticmethod
    def forward(ctx, feature, index, weight):
        (f, w), f64 = _pn2_float("feature_interpolate", feature, weight)
        _dev(index)
        if index.dtype != torch.int64:
            raise RuntimeError("feature_interpolate: index must be int64")
        if f.dim() != 3 or index.dim() != 3 or index.shape[2] != 3 or tuple(w.shape) != tuple(index.shape) \
                or index.shape[0] != f.shape[0]:
            raise RuntimeError("feature_interpolate: expected feature (B,C,N1), index (B,N2,3) and weight (B,N2,3)")
        index = index.contiguous()
        B, Cc, N1 = f.shape
        N2 = index.shape[1]
        out = torch.empty((B, Cc, N2), device=f.device, dtype=f.dtype)
        fn = lib().mvk_interpolate_fwd_f64 if f64 else lib().mvk_interpolate_fwd
        check(fn(_p(f), _p(index), _p(w), B, Cc, N1, N2, _p(out), _p(pn2_index_status(f.device)), _stream()))
        if _PN2_EAGER_CHECK[0]:
            pn2_check_indices(f.device)
        ctx.save_for_backward(index, w)
        ctx.n1, ctx.f64 = N1, f64
        ctx.det = is_deterministic()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        index, w = ctx.saved_tensors
        g = grad_out.to(w.dtype).contiguous()
        B, Cc, N2 = g.shape
        if ctx.det:
            row_start, entries = index_csr(index, ctx.n1, pn2_index_status(g.device))
            gi = torch.empty((B, Cc, ctx.n1), device=g.device, dtype=g.dtype)       # every element is written
            fn = lib().mvk_interpolate_bwd_csr_f64 if ctx.f64 else lib().mvk_interpolate_bwd_csr
            check(fn(_p(g), _p(w), _p(row_start), _p(entries), B, Cc, ctx.n1, N2, _p(gi), _stream()))
            return gi, None, None
        gi = torch.zeros((B, Cc, ctx.n1), device=g.device, dtype=g.dtype)
        fn = lib().mvk_interpolate_bwd_f64 if ctx.f64 else lib().mvk_interpolate_bwd
        check(fn(_p(g), _p(index), _p(w), B, Cc, ctx.n1, N2, _p(gi), _p(pn2_index_status(g.device)), _stream()))
        return gi, None, None


def feature_interpolate(feature, index, weight):
    """feature (B,C,N1), index (B,N2,3) int64, weight (B,N2,3) -> (B,C,N2) (mvpnet/ops/interpolate.py:23-35)."""
    return _FeatureInterpolateFn.apply(feature, index, weight)


# --------------------------------------------------------------------------------------------
# MVPNet baseline, frozen inference: group / interpolate, shared MLP and max in one launch (csrc/pn2_mlp.hip)
# --------------------------------------------------------------------------------------------

def pn2_mlp_supported(widths):
    """Whether the fused chain kernels take these widths (input width, then one per layer): the library's own rule
    (mvk_pn2_mlp_supported, a host function, no GPU call) -- at most three layers, input rows of at most 768 values,
    layers of at most 512, and the two activation buffers of a 32-row tile within 160 KiB of LDS."""
    widths = [int(w) for w in widths]
    if len(widths) < 2:
        return False
    return bool(lib().mvk_pn2_mlp_supported((C.c_int * len(widths))(*widths), len(widths) - 1))


def _pn2_mlp_args(name, floats, index, params, widths):
    """The refusals shared by pn2_sa_mlp_max and pn2_fp_mlp (dtype, layout and autograd first, then residence, so each
    can be told apart on any tensor); returns the widths as a list and as the host array of the C call."""
    for t in list(floats) + [params]:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError("%s: floating operands must be float32 (got %s)" % (name, t.dtype))
        if not t.is_contiguous():
            raise RuntimeError("%s: operands must be contiguous" % name)
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("%s has no backward: call it under torch.no_grad() or on detached tensors" % name)
    if index is not None:
        if index.dtype != torch.int64:
            raise RuntimeError("%s: index must be int64" % name)
        if not index.is_contiguous():
            raise RuntimeError("%s: operands must be contiguous" % name)
    _dev(index, params, *floats)
    widths = [int(w) for w in widths]
    if len(widths) < 2 or min(widths) < 1:
        raise RuntimeError("%s: widths must hold the input width and one positive width per layer" % name)
    need = sum(widths[l + 1] * (widths[l] + 1) for l in range(len(widths) - 1))
    if params.dim() != 1 or params.numel() != need:
        raise RuntimeError("%s: params must be the packed chain [W0|b0|W1|b1|...] of %d values for widths %s (got %s)"
                           % (name, need, widths, tuple(params.shape)))
    return widths, (C.c_int * len(widths))(*widths)


def pn2_sa_mlp_max(xyz, feature, new_xyz, index, params, widths):
    """A frozen SetAbstraction after its ball query, as one launch: xyz (B,3,N), feature (B,C,N) or None, new_xyz (B,3,M),
    index (B,M,K) int64 -> (B,widths[-1],M), the maximum over k of the chain relu(W_l x + b_l) applied to the row
    [feature[:, index] | xyz[:, index] - new_xyz]. The row holds the coordinates when widths[0] == C + 3 and the features
    alone when widths[0] == C. params: the packed float32 chain [W0|b0|W1|b1|...], W_l (widths[l+1], widths[l]); at most
    three layers. An index outside [0, N) reads as zero before the centroid is subtracted, like group_points. No
    autograd, no host synchronisation, no allocation but the output."""
    widths, w_host = _pn2_mlp_args("pn2_sa_mlp_max", (xyz, feature, new_xyz), index, params, widths)
    if xyz.dim() != 3 or xyz.shape[1] != 3 or new_xyz.dim() != 3 or new_xyz.shape[1] != 3 or index.dim() != 3 \
            or new_xyz.shape[0] != xyz.shape[0] or tuple(index.shape[:2]) != (xyz.shape[0], new_xyz.shape[2]) \
            or (feature is not None and (feature.dim() != 3 or feature.shape[0] != xyz.shape[0]
                                         or feature.shape[2] != xyz.shape[2])):
        raise RuntimeError("pn2_sa_mlp_max: expected xyz (B,3,N), feature (B,C,N) or None, new_xyz (B,3,M), index (B,M,K)")
    B, _, N = xyz.shape
    M, K = index.shape[1], index.shape[2]
    Cf = feature.shape[1] if feature is not None else 0
    if widths[0] not in ((Cf + 3, Cf) if Cf else (3,)):
        raise RuntimeError("pn2_sa_mlp_max: widths[0] = %d, the input rows hold %d features (+ 3 coordinates)"
                           % (widths[0], Cf))
    out = torch.empty((B, widths[-1], M), device=xyz.device, dtype=torch.float32)
    check(lib().mvk_pn2_sa_fwd(_p(xyz), _p(feature), _p(new_xyz), _p(index), _p(params), w_host, len(widths) - 1, B, Cf,
                               int(widths[0] == Cf + 3), N, M, K, _p(out), _stream()))
    return out


def pn2_fp_mlp(sparse, index, weight, dense, params, widths, relu_last=True):
    """A frozen FeaturePropagation after its 3-NN search, or a plain shared MLP, as one launch: sparse (B,C2,N2), index
    (B,N1,3) int64, weight (B,N1,3), dense (B,C1,N1) or None -> (B,widths[-1],N1), the chain applied to the row
    [interpolated (C2) | dense (C1)]; the interpolated values are feature_interpolate's bit for bit. index None: the row
    is `dense` alone (sparse and weight are ignored). relu_last False: the last layer is linear (logits). params, widths
    and the rest as pn2_sa_mlp_max."""
    if index is None:
        sparse = weight = None
    widths, w_host = _pn2_mlp_args("pn2_fp_mlp", (sparse, weight, dense), index, params, widths)
    if index is None:
        if dense is None or dense.dim() != 3:
            raise RuntimeError("pn2_fp_mlp: without an index, dense (B,C1,N1) is the input")
        B, C2, N2 = dense.shape[0], 0, 0
    else:
        if sparse is None or weight is None or sparse.dim() != 3 or index.dim() != 3 or index.shape[2] != 3 \
                or tuple(weight.shape) != tuple(index.shape) or index.shape[0] != sparse.shape[0] \
                or (dense is not None and (dense.dim() != 3 or dense.shape[0] != sparse.shape[0]
                                           or dense.shape[2] != index.shape[1])):
            raise RuntimeError("pn2_fp_mlp: expected sparse (B,C2,N2), index (B,N1,3), weight (B,N1,3), dense (B,C1,N1) "
                               "or None")
        B, C2, N2 = sparse.shape
    N1 = index.shape[1] if index is not None else dense.shape[2]
    C1 = dense.shape[1] if dense is not None else 0
    if widths[0] != C2 + C1:
        raise RuntimeError("pn2_fp_mlp: widths[0] = %d, the input rows hold %d + %d values" % (widths[0], C2, C1))
    dev = dense.device if dense is not None else sparse.device
    out = torch.empty((B, widths[-1], N1), device=dev, dtype=torch.float32)
    status = pn2_index_status(dev) if index is not None else None
    check(lib().mvk_pn2_fp_fwd(_p(sparse), _p(index), _p(weight), _p(dense), _p(params), w_host, len(widths) - 1,
                               int(bool(relu_last)), B, C2, C1, N2, N1, _p(out), _p(status), _stream()))
    return out


def pn2_fa_mlp(feature_2d, image_xyz, points, index, params, widths, reduction='sum', use_relation=True, lengths=None):
    """A frozen FeatureAggregation fed from the 2D encoder's map, as one launch: feature_2d (B*nv,C,h,w), contiguous or
    channels-last and read in place, image_xyz (B,nv,h,w,3), points (B,3,N), index (B,N,K) int64 flat pixel indices
    view*h*w + pixel -> (B,widths[-1],N), the sum (or max) over k of the chain applied to the row [feature_2d at the
    pixel | image_xyz at the pixel - point | squared distance]; the features alone with use_relation False. An index
    outside [0, nv*h*w) reads as zero before the point is subtracted, like group_points. lengths: int64 (B,) on the
    device, for a padded batch: columns >= lengths[b] (clamped to [1, N]) of element b come out as zeros, and their
    indices and points are never read. K <= 128. params, widths and the rest as pn2_sa_mlp_max."""
    name = "pn2_fa_mlp"
    if feature_2d.dtype != torch.float32:
        raise RuntimeError("%s: floating operands must be float32 (got %s)" % (name, feature_2d.dtype))
    if feature_2d.dim() != 4:
        raise RuntimeError("%s: expected feature_2d (B*nv,C,h,w)" % name)
    channels_last = not feature_2d.is_contiguous()
    if channels_last and not feature_2d.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError("%s: feature_2d must be contiguous or channels-last" % name)
    if feature_2d.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("%s has no backward: call it under torch.no_grad() or on detached tensors" % name)
    if reduction not in ('sum', 'max'):
        raise RuntimeError("%s: reduction must be 'sum' or 'max', got %r" % (name, reduction))
    if image_xyz.dim() != 5 or image_xyz.shape[4] != 3 or points.dim() != 3 or points.shape[1] != 3 or index.dim() != 3 \
            or points.shape[0] != image_xyz.shape[0] or tuple(index.shape[:2]) != (points.shape[0], points.shape[2]) \
            or tuple(image_xyz.shape[2:4]) != tuple(feature_2d.shape[2:]):
        raise RuntimeError("%s: expected feature_2d (B*nv,C,h,w), image_xyz (B,nv,h,w,3), points (B,3,N), index (B,N,K)"
                           % name)
    B, nv, h, w = image_xyz.shape[:4]
    Cf, N, K = feature_2d.shape[1], points.shape[2], index.shape[2]
    if feature_2d.shape[0] != B * nv:
        raise RuntimeError("%s: feature_2d holds %d images, image_xyz has %d x %d views" % (name, feature_2d.shape[0], B, nv))
    rows = Cf + (4 if use_relation else 0)
    if len(widths) and int(widths[0]) != rows:
        raise RuntimeError("%s: widths[0] = %d, the input rows hold %d values" % (name, int(widths[0]), rows))
    if lengths is not None:
        lengths = _pn2_lengths(name, lengths, points)
    widths, w_host = _pn2_mlp_args(name, (image_xyz, points), index, params, widths)
    _dev(feature_2d)
    hw = h * w
    strides = (Cf * hw, 1, Cf) if channels_last else (Cf * hw, hw, 1)
    out = torch.empty((B, widths[-1], N), device=points.device, dtype=torch.float32)
    check(lib().mvk_pn2_fa_fwd(_p(feature_2d), strides[0], strides[1], strides[2], _p(image_xyz), _p(points), _p(index),
                               _p(lengths), _p(params), w_host, len(widths) - 1, B, nv, Cf, hw, N, K,
                               int(bool(use_relation)), int(reduction == 'max'), _p(out), _stream()))
    return out


# --------------------------------------------------------------------------------------------
# MVPNet baseline, training mode: group rows and the max over the neighbours (csrc/pn2_rows.hip)
# --------------------------------------------------------------------------------------------

def _pn2_train_args(name, floats, index=None):
    """The refusals shared by pn2_sa_rows and pn2_rows_max (dtype and layout first, then residence, like _pn2_mlp_args)."""
    for t in floats:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError("%s: floating operands must be float32 (got %s)" % (name, t.dtype))
        if not t.is_contiguous():
            raise RuntimeError("%s: operands must be contiguous" % name)
    if index is not None:
        if index.dtype != torch.int64:
            raise RuntimeError("%s: index must be int64" % name)
        if not index.is_contiguous():
            raise RuntimeError("%s: operands must be contiguous" % name)
    _dev(index, *floats)


def _pn2_rows_reduce_args(name, y, B, M, K):
    """The refusals shared by pn2_rows_max and pn2_rows_sum; returns B, M, K as ints."""
    _pn2_train_args(name, (y,))
    B, M, K = int(B), int(M), int(K)
    if y.dim() != 2 or B < 0 or M < 0 or K < 1 or y.shape[0] != B * M * K:
        raise RuntimeError("%s: expected y (B*M*K, Cout) with K >= 1, got %s for B=%d M=%d K=%d"
                           % (name, tuple(y.shape), B, M, K))
    if y.shape[0] >= 1 << 31:
        raise RuntimeError("%s: B*M*K = %d rows must be below 2^31" % (name, y.shape[0]))
    return B, M, K


class _PN2SaRowsFn(torch.autograd.Function):
    """X [Cin, B*M*K] of a ball-query group; the gradient goes to the features alone. The backward is a float-atomic
    scatter-add by default; when set_deterministic was on in the forward it is the ordered gather over the transposed
    index, the CSR kept under the CALLER's index tensor like _GroupPointsFn's (one CSR for both ops on one index)."""

    @staticmethod
    def forward(ctx, xyz, feature, new_xyz, index, use_xyz):
        B, _, N = xyz.shape
        M, K = index.shape[1], index.shape[2]
        Cf = feature.shape[1] if feature is not None else 0
        use_xyz = bool(use_xyz) or feature is None
        X = torch.empty((Cf + (3 if use_xyz else 0), B * M * K), device=xyz.device, dtype=torch.float32)
        check(lib().mvk_pn2_sa_rows_fwd(_p(xyz), _p(feature), _p(new_xyz), _p(index), B, Cf, int(use_xyz), N, M, K, _p(X),
                                        _stream()))
        ctx.save_for_backward(index)
        ctx.dims = (B, Cf, N, M, K)
        ctx.det, ctx.csr_owner = is_deterministic(), index
        return X

    @staticmethod
    def backward(ctx, grad_x):
        (index,) = ctx.saved_tensors
        B, Cf, N, M, K = ctx.dims
        if Cf == 0 or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        g = _f32c(grad_x)
        if ctx.det:
            row_start, entries = _index_csr_shared(ctx.csr_owner, index, N)
            gf = torch.empty((B, Cf, N), device=g.device, dtype=torch.float32)          # every element is written
            check(lib().mvk_pn2_sa_rows_bwd_csr(_p(g), _p(row_start), _p(entries), B, Cf, N, M, K, _p(gf), _stream()))
            return None, gf, None, None, None
        gf = torch.zeros((B, Cf, N), device=g.device, dtype=torch.float32)
        check(lib().mvk_pn2_sa_rows_bwd(_p(g), _p(index), B, Cf, N, M, K, _p(gf), _stream()))
        return None, gf, None, None, None


def pn2_sa_rows(xyz, feature, new_xyz, index, use_xyz=True):
    """The input rows of a SetAbstraction's shared MLP after its ball query, as the transposed operand of ops.linear:
    xyz (B,3,N), feature (B,C,N) or None, new_xyz (B,3,M), index (B,M,K) int64 -> X (Cin, B*M*K) channel-major, column
    (b*M + m)*K + k = [feature[b, :, j] | xyz[b, :, j] - new_xyz[b, :, m]] with j = index[b, m, k] (QueryGrouper's order);
    the coordinates alone without features, the features alone with use_xyz False. An index outside [0, N) reads as zero
    before the centroid is subtracted, like group_points. Differentiable in `feature` only (atomic scatter-add, or the
    ordered per-key sums when set_deterministic was on in the forward); coordinates that require a gradient are refused.
    One launch, no host synchronisation."""
    _pn2_train_args("pn2_sa_rows", (xyz, feature, new_xyz), index)
    if xyz.dim() != 3 or xyz.shape[1] != 3 or new_xyz.dim() != 3 or new_xyz.shape[1] != 3 or index.dim() != 3 \
            or new_xyz.shape[0] != xyz.shape[0] or tuple(index.shape[:2]) != (xyz.shape[0], new_xyz.shape[2]) \
            or (feature is not None and (feature.dim() != 3 or feature.shape[0] != xyz.shape[0]
                                         or feature.shape[2] != xyz.shape[2])):
        raise RuntimeError("pn2_sa_rows: expected xyz (B,3,N), feature (B,C,N) or None, new_xyz (B,3,M), index (B,M,K)")
    if torch.is_grad_enabled() and (xyz.requires_grad or new_xyz.requires_grad):
        raise RuntimeError("pn2_sa_rows has no gradient for coordinates: pass xyz and new_xyz detached")
    if index.numel() >= 1 << 31:
        raise RuntimeError("pn2_sa_rows: B*M*K = %d rows must be below 2^31" % index.numel())
    return _PN2SaRowsFn.apply(xyz, feature, new_xyz, index, use_xyz)


class _PN2RowsMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, B, M, K):
        Cout = y.shape[1]
        out = torch.empty((B, Cout, M), device=y.device, dtype=torch.float32)
        arg = torch.empty((B, Cout, M), device=y.device, dtype=torch.int32)
        check(lib().mvk_pn2_rows_max_fwd(_p(y), B, M, K, Cout, _p(out), _p(arg), _stream()))
        ctx.save_for_backward(arg)
        ctx.dims = (B, M, K, Cout)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _g_arg=None):
        (arg,) = ctx.saved_tensors
        B, M, K, Cout = ctx.dims
        g = _f32c(g)
        dy = torch.empty((B * M * K, Cout), device=g.device, dtype=torch.float32)       # every element is written
        check(lib().mvk_pn2_rows_max_bwd(_p(g), _p(arg), B, M, K, Cout, _p(dy), _stream()))
        return dy, None, None, None


def pn2_rows_max(y, B, M, K, return_arg=False):
    """The max over the neighbours on rows: y (B*M*K, Cout) row-major, row (b*M + m)*K + k (what ops.bn_lrelu returns)
    -> (B, Cout, M), the layout the next level reads. Among equal maxima the smallest k is the one that receives the
    gradient (a ball query pads its rows with copies of the first hit); a NaN propagates as in torch.max. return_arg:
    also that k, int32 (B, Cout, M). One launch forward, one backward (every element of the gradient is written: no zero
    fill, no atomics)."""
    B, M, K = _pn2_rows_reduce_args("pn2_rows_max", y, B, M, K)
    out, arg = _PN2RowsMaxFn.apply(y, B, M, K)
    return (out, arg) if return_arg else out


# --------------------------------------------------------------------------------------------
# MVPNet baseline, training mode: the 2D -> 3D hand-off around FeatureAggregation's shared MLP (csrc/pn2_rows.hip,
# DESIGN 7o)
# --------------------------------------------------------------------------------------------

class _PN2FaRowsFn(torch.autograd.Function):
    """X [C (+4), B*N*K] of a batch of aggregation rows; the gradient goes to the encoder's map alone, in the map's own
    memory format. Atomic scatter-add by default; when set_deterministic was on in the forward, the ordered gather over
    the transposed index with nv*h*w keys, the CSR kept under the CALLER's index tensor like _GroupPointsFn's."""

    @staticmethod
    def forward(ctx, feature_2d, image_xyz, points, index, use_relation):
        B, nv, h, w = image_xyz.shape[:4]
        Cf, N, K = feature_2d.shape[1], points.shape[2], index.shape[2]
        hw = h * w
        channels_last = not feature_2d.is_contiguous()
        strides = (Cf * hw, 1, Cf) if channels_last else (Cf * hw, hw, 1)
        X = torch.empty((Cf + (4 if use_relation else 0), B * N * K), device=points.device, dtype=torch.float32)
        check(lib().mvk_pn2_fa_rows_fwd(_p(feature_2d), strides[0], strides[1], strides[2], _p(image_xyz), _p(points),
                                        _p(index), B, nv, Cf, hw, N, K, int(use_relation), _p(X), _stream()))
        ctx.save_for_backward(index)
        ctx.dims, ctx.strides, ctx.channels_last = (B, nv, Cf, h, w, N, K), strides, channels_last
        ctx.det, ctx.csr_owner = is_deterministic(), index
        return X

    @staticmethod
    def backward(ctx, grad_x):
        (index,) = ctx.saved_tensors
        B, nv, Cf, h, w, N, K = ctx.dims
        if Cf == 0 or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = _f32c(grad_x)
        fmt = torch.channels_last if ctx.channels_last else torch.contiguous_format
        si, sc, sp = ctx.strides
        if ctx.det:
            row_start, entries = _index_csr_shared(ctx.csr_owner, index, nv * h * w)
            gm = torch.empty((B * nv, Cf, h, w), device=g.device, dtype=torch.float32, memory_format=fmt)   # all written
            check(lib().mvk_pn2_fa_rows_bwd_csr(_p(g), _p(row_start), _p(entries), B, nv, Cf, h * w, N, K, _p(gm), si, sc,
                                                sp, _stream()))
            return gm, None, None, None, None
        gm = torch.empty((B * nv, Cf, h, w), device=g.device, dtype=torch.float32, memory_format=fmt).zero_()
        check(lib().mvk_pn2_fa_rows_bwd(_p(g), _p(index), B, nv, Cf, h * w, N, K, _p(gm), si, sc, sp, _stream()))
        return gm, None, None, None, None


def pn2_fa_rows(feature_2d, image_xyz, points, index, use_relation=True):
    """The input rows of FeatureAggregation's shared MLP for a batch, straight from the 2D encoder's map, as the
    transposed operand of ops.linear: feature_2d (B*nv,C,h,w), contiguous or channels-last and read in place, image_xyz
    (B,nv,h,w,3), points (B,3,N), index (B,N,K) int64 flat pixel indices view*h*w + pixel -> X (C+4, B*N*K)
    channel-major, column (b*N + n)*K + k = [feature_2d at the pixel | image_xyz at the pixel - point | squared
    distance]; the features alone, (C, B*N*K), with use_relation False. An index outside [0, nv*h*w) reads as zero before
    the point is subtracted, like the two group_points calls of MVPNet3D.forward. Differentiable in feature_2d only
    (atomic scatter-add, or the ordered per-pixel sums when set_deterministic was on in the forward; the gradient has the
    map's memory format); image_xyz or points that require a gradient are refused. One launch, no host synchronisation."""
    name = "pn2_fa_rows"
    if feature_2d.dtype != torch.float32:
        raise RuntimeError("%s: floating operands must be float32 (got %s)" % (name, feature_2d.dtype))
    if feature_2d.dim() != 4:
        raise RuntimeError("%s: expected feature_2d (B*nv,C,h,w)" % name)
    if not (feature_2d.is_contiguous() or feature_2d.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("%s: feature_2d must be contiguous or channels-last" % name)
    _pn2_train_args(name, (image_xyz, points), index)
    _dev(feature_2d)
    if image_xyz.dim() != 5 or image_xyz.shape[4] != 3 or points.dim() != 3 or points.shape[1] != 3 or index.dim() != 3 \
            or points.shape[0] != image_xyz.shape[0] or tuple(index.shape[:2]) != (points.shape[0], points.shape[2]) \
            or tuple(image_xyz.shape[2:4]) != tuple(feature_2d.shape[2:]):
        raise RuntimeError("%s: expected feature_2d (B*nv,C,h,w), image_xyz (B,nv,h,w,3), points (B,3,N), index (B,N,K)"
                           % name)
    B, nv, h, w = image_xyz.shape[:4]
    if feature_2d.shape[0] != B * nv:
        raise RuntimeError("%s: feature_2d holds %d images, image_xyz has %d x %d views" % (name, feature_2d.shape[0], B, nv))
    if torch.is_grad_enabled() and (image_xyz.requires_grad or points.requires_grad):
        raise RuntimeError("%s has no gradient for coordinates: pass image_xyz and points detached" % name)
    if index.numel() >= 1 << 31 or B * nv * h * w >= 1 << 31:
        raise RuntimeError("%s: B*N*K = %d rows and B*nv*h*w = %d pixels must be below 2^31"
                           % (name, index.numel(), B * nv * h * w))
    return _PN2FaRowsFn.apply(feature_2d, image_xyz, points, index, bool(use_relation))


class _PN2RowsSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, B, M, K):
        Cout = y.shape[1]
        out = torch.empty((B, Cout, M), device=y.device, dtype=torch.float32)
        check(lib().mvk_pn2_rows_sum_fwd(_p(y), B, M, K, Cout, _p(out), _stream()))
        ctx.dims = (B, M, K, Cout)
        return out

    @staticmethod
    def backward(ctx, g):
        B, M, K, Cout = ctx.dims
        g = _f32c(g)
        dy = torch.empty((B * M * K, Cout), device=g.device, dtype=torch.float32)       # every element is written
        check(lib().mvk_pn2_rows_sum_bwd(_p(g), B, M, K, Cout, _p(dy), _stream()))
        return dy, None, None, None


def pn2_rows_sum(y, B, M, K):
    """The sum over the neighbours on rows: y (B*M*K, Cout) row-major, row (b*M + m)*K + k (what ops.bn_lrelu returns)
    -> (B, Cout, M): the first row's value, then one rounded float32 addition per further row in ascending k. One launch
    forward, one backward (every element of the gradient is written: no zero fill, no atomics)."""
    B, M, K = _pn2_rows_reduce_args("pn2_rows_sum", y, B, M, K)
    return _PN2RowsSumFn.apply(y, B, M, K)


# --------------------------------------------------------------------------------------------
# fused FeatureAggregation path: gather kernel + MFMA linear layers
# --------------------------------------------------------------------------------------------

def fa_gather(feature_2d, image_xyz, knn, points):
    """X [C+4, np*k] channel-major for ONE sphere: feature_2d (nv,C,h,w) f32, image_xyz (nv,h,w,3) f32,
    knn (np,k) int64 flat pixel indices, points (np,3) f32. Treated as a constant by autograd (the 2D
    encoder is frozen in every MV-KPConv variant, architectures_sphere.py:234-237)."""
    _dev(feature_2d, image_xyz, knn, points)
    f = feature_2d.detach()
    # the frozen encoder's convolutions deliver channels-last maps: read in place (no NCHW copy of the map)
    cl = (f.dim() == 4 and f.dtype == torch.float32 and not f.is_contiguous()
          and f.is_contiguous(memory_format=torch.channels_last))
    if not cl:
        f = _f32c(f)
    xyz, pts = _f32c(image_xyz), _f32c(points)
    knn = knn.contiguous()
    if knn.dtype != torch.int64:
        raise RuntimeError("fa_gather: knn must be int64")
    nv, Cc, h, w = f.shape
    np_, k = knn.shape
    X = torch.empty((Cc + 4, np_ * k), device=f.device, dtype=torch.float32)
    check(lib().mvk_fa_gather_fwd_ex(_p(f), int(cl), _p(xyz), _p(knn), _p(pts), Cc, nv, h * w, np_, k, _p(X), _stream()))
    return X


class _LinearFn(torch.autograd.Function):
    """y = x @ W^T on the f32 MFMA GEMM. x is [M,Kd] row-major, or [Kd,M] when x_is_transposed.
    passthrough: also returns x itself as a second (aliasing) output for a parallel consumer of x -- the shortcut of a
    residual block; the backward then ACCUMULATES g @ W into that consumer's gradient inside the GEMM (its epilogue adds
    onto the buffer) instead of leaving autograd to sum two tensors with one more launch per block."""

    @staticmethod
    def forward(ctx, x, W, x_is_transposed, stats_n_valid=None, passthrough=False, finish=None, a_transform=None):
        ctx.save_for_backward(x, W)
        ctx.xt = bool(x_is_transposed)
        ctx.set_materialize_grads(False)    # no zero tensors for unused gradients (statistics, an unused passthrough)
        alias = x.view_as(x) if passthrough else None
        y, st = _product(x, W, transA=ctx.xt, transB=True, stats_n_valid=stats_n_valid, finish=finish,
                         a_transform=a_transform)
        if st is not None:
            ctx.mark_non_differentiable(st.partials)
        return y, st, alias

    @staticmethod
    def backward(ctx, g, g_st=None, g_alias=None):
        x, W = ctx.saved_tensors
        if g is None:
            return g_alias, None, None, None, None, None, None
        g = _f32c(g)
        dx = dW = None
        if ctx.needs_input_grad[0]:
            if ctx.xt:
                dx = gemm(W, g, transA=True, transB=True)                    # [Kd,M]
                if g_alias is not None:
                    dx = dx + g_alias
            elif (g_alias is not None and g_alias.dtype == torch.float32 and g_alias.is_contiguous()
                  and g_alias.shape == (g.shape[0], W.shape[1]) and _accumulate_in_place_ok(g_alias)):
                # the parallel consumer's gradient is this node's own grad input and no pending product reads it: add onto it
                dx = gemm(g, W, out=g_alias, accumulate=True)
            else:
                dx = gemm(g, W)                                              # [M,Kd]
                if g_alias is not None:
                    dx = dx + g_alias
        if ctx.needs_input_grad[1]:
            # dW [N,Kd] = g^T [N,M] @ x [M,Kd]
            dW = _dw_gemm(g, x, transB=ctx.xt, target=W)
        return dx, dW, None, None, None, None, None


def gemm_dual(A, B, A2, B2):
    """A @ B + A2 @ B2 (all row-major, same output shape) in one launch with the two reductions laid end to end
    (mvk_gemm_f32_dual), or None when the shape is not supported (the caller runs two products)."""
    _dev(A, B, A2, B2)
    A, B, A2, B2 = _f32c(A), _f32c(B), _f32c(A2), _f32c(B2)
    M, Kd = A.shape
    N, Kd2 = B.shape[1], A2.shape[1]
    if A2.shape[0] != M or B.shape[0] != Kd or B2.shape != (Kd2, N):
        raise RuntimeError("gemm_dual: shapes do not match")
    split_arena_prepare(A.device)
    split = C.c_int(0)
    check(lib().mvk_gemm_f32_dual_plan(M, N, Kd, Kd2, C.byref(split)))
    if split.value == 0:
        return None
    out = _split_out((M, N), A.device, split.value)
    check(lib().mvk_gemm_f32_dual(_p(A), _p(B), _p(A2), _p(B2), _p(out), M, N, Kd, Kd2, _stream()))
    return out


class _LinearPairFn(torch.autograd.Function):
    """(x W0^T, x W1^T) in one launch (mvk_gemm_f32_pair): unary1 and the shortcut layer of a bottleneck block read the
    same input. The backward is the two layers' own: dx = g0 W0 + g1 W1 (the second product accumulates onto the first),
    the weight gradients go through _dw_gemm like every other layer's."""

    @staticmethod
    def forward(ctx, x, W0, W1, stats_n_valid, plan, finish):
        M, Kd = x.shape
        N0, N1 = W0.shape[0], W1.shape[0]
        _, s0, s1, r0, r1 = plan
        want = r0 > 0 or r1 > 0
        outs, parts = [], []
        for N, sp, rows in ((N0, s0, r0), (N1, s1, r1)):
            outs.append(_split_out((M, N), x.device, sp))
            parts.append(torch.empty(((M + rows - 1) // rows, 2, N), device=x.device, dtype=torch.float32) if rows > 0 else None)
        fins, done = [None, None], [None, None]
        for i, (bn, part, N) in enumerate(((finish[0], parts[0], N0), (finish[1], parts[1], N1))):
            if bn is not None and part is not None:
                fins[i], done[i] = _fin_struct(bn, N, x.device)
        if fins[0] is not None or fins[1] is not None:
            check(lib().mvk_gemm_f32_pair_bn(_p(x), _p(W0), _p(W1), _p(outs[0]), _p(outs[1]), M, N0, N1, Kd, 1,
                                             _p(parts[0]), _p(parts[1]), _p(stats_n_valid),
                                             C.byref(fins[0]) if fins[0] is not None else None,
                                             C.byref(fins[1]) if fins[1] is not None else None, _stream()))
        else:
            check(lib().mvk_gemm_f32_pair(_p(x), _p(W0), _p(W1), _p(outs[0]), _p(outs[1]), M, N0, N1, Kd, 1, int(want),
                                          _p(parts[0]), _p(parts[1]), _p(stats_n_valid) if want else None, _stream()))
        ctx.save_for_backward(x, W0, W1)
        ctx.set_materialize_grads(False)
        for part in parts:
            if part is not None:
                ctx.mark_non_differentiable(part)
        st0, st1 = [BnStats(p, r, d) if p is not None else None for p, r, d in zip(parts, (r0, r1), done)]
        return outs[0], st0, outs[1], st1

    @staticmethod
    def backward(ctx, g0, g_st0, g1, g_st1):
        x, W0, W1 = ctx.saved_tensors
        dx = dW0 = dW1 = None
        g0 = _f32c(g0) if g0 is not None else None
        g1 = _f32c(g1) if g1 is not None else None
        if ctx.needs_input_grad[0]:
            if g0 is not None and g1 is not None:
                dx = gemm_dual(g0, W0, g1, W1)          # g0 W0 + g1 W1 as one launch, or None
            if dx is None:
                if g0 is not None:
                    dx = gemm(g0, W0)
                if g1 is not None:
                    dx = gemm(g1, W1, out=dx, accumulate=True) if dx is not None else gemm(g1, W1)
        if ctx.needs_input_grad[1] and g0 is not None:
            dW0 = _dw_gemm(g0, x, target=W0)
        if ctx.needs_input_grad[2] and g1 is not None:
            dW1 = _dw_gemm(g1, x, target=W1)
        return dx, dW0, dW1, None, None, None


def linear_pair(x, W0, W1, stats_n_valid=None, bn0=None, bn1=None):
    """(linear(x, W0), linear(x, W1)) in one launch, or None when the two products cannot share one (different tile
    classes: the caller then runs them one after the other). Outputs carry their BatchNorm statistics like linear()'s."""
    _dev(x, W0, W1, stats_n_valid)
    if x.dtype != torch.float32 or not x.is_contiguous() or W0.dtype != torch.float32 or W1.dtype != torch.float32 \
            or not W0.is_contiguous() or not W1.is_contiguous() or x.dim() != 2 or x.shape[0] == 0:
        return None
    M, Kd = x.shape
    split_arena_prepare(x.device)
    fold = BN_FOLD and (bn0 is not None or bn1 is not None)       # finished statistics: the epilogue whatever the row count
    want = stats_n_valid is not None and M <= _STATS_EPILOGUE_ROWS and \
        (fold or (M > bn_single_launch_rows(W0.shape[0]) and M > bn_single_launch_rows(W1.shape[0])))
    plan = (C.c_int * 5)()
    check(lib().mvk_gemm_f32_pair_plan(M, W0.shape[0], W1.shape[0], Kd, int(want), plan))
    if not plan[0]:
        return None
    plan = tuple(int(v) for v in plan)
    y0, st0, y1, st1 = _LinearPairFn.apply(x, W0, W1, stats_n_valid if want else None, plan,
                                           tuple(bn if _finishable(bn) else None for bn in (bn0, bn1)))
    if st0 is not None:
        y0._mvk_bn_stats = st0
    if st1 is not None:
        y1._mvk_bn_stats = st1
    return y0, y1


def linear(x, W, x_is_transposed=False, stats_n_valid=None, passthrough=False, bn=None, _a_transform=None):
    """nn.Linear without bias / a 1x1 convolution over rows, on gemm_f32_mfma. stats_n_valid: see kpconv().
    passthrough=True returns (y, x') with x' an alias of x whose gradient is summed into x's inside the backward GEMM
    (use x' for the other consumer of x). bn: the nn.BatchNorm1d that follows (statistics finished by the product).
    _a_transform: bn_lrelu_linear's operand transform (x is then its lazy tensor)."""
    y, st, alias = _LinearFn.apply(x, W, x_is_transposed, stats_n_valid, passthrough,
                                   bn if stats_n_valid is not None and _finishable(bn) else None, _a_transform)
    if st is not None:
        y._mvk_bn_stats = st
    return (y, alias) if passthrough else y


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, lut, weight):
        _dev(logits, labels, lut, weight)
        logits = _f32c(logits)
        if labels.dtype not in (torch.int32, torch.int64):
            labels = labels.long()
        labels = labels.contiguous()
        N, Cc = logits.shape
        part = torch.empty((lib().mvk_xent_workspace_floats(N),), device=logits.device, dtype=torch.float32)
        out2 = torch.empty((2,), device=logits.device, dtype=torch.float32)
        check(lib().mvk_xent_fwd(_p(logits), N, Cc, _p(labels), int(labels.dtype == torch.int64), _p(lut), lut.numel(),
                                 _p(weight), _p(part), _p(out2), _stream()))
        ctx.save_for_backward(logits, labels, lut, weight, out2)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        logits, labels, lut, weight, out2 = ctx.saved_tensors
        g = _f32c(g)
        d = torch.empty_like(logits)
        check(lib().mvk_xent_bwd(_p(logits), logits.shape[0], logits.shape[1], _p(labels),
                                 int(labels.dtype == torch.int64), _p(lut), lut.numel(), _p(weight), _p(out2), _p(g), _p(d),
                                 _stream()))
        return d, None, None, None


def cross_entropy_lut(logits, labels, lut, class_weight=None):
    """KPFCNN's segmentation loss (architectures.py:345-372) as one autograd node, three launches forward + backward:
    labels [N] (int32 / int64, raw dataset values) are renumbered through `lut` (int32: lut[l + 1] = class of label
    l or -1 = ignored; lut[0] for negative labels, lut[-1] for labels above the table), then the class-weighted
    cross entropy of logits [N, C], mean over the kept points (torch.nn.CrossEntropyLoss(weight, ignore_index=-1))."""
    if lut.dtype != torch.int32 or lut.dim() != 1 or lut.numel() < 3:
        raise RuntimeError("cross_entropy_lut: lut must be a 1-D int32 tensor of at least 3 entries")
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise RuntimeError("cross_entropy_lut: logits [N, C] and labels [N] expected")
    if class_weight is not None and (class_weight.dtype != torch.float32 or class_weight.numel() != logits.shape[1]):
        raise RuntimeError("cross_entropy_lut: class_weight must be float32 [C]")
    return _XentFn.apply(logits, labels, lut, None if class_weight is None else class_weight.contiguous())


# --------------------------------------------------------------------------------------------
# MVPNet baseline: segmentation loss and metrics on channel-first logits (csrc/loss.hip, seg_*)
# --------------------------------------------------------------------------------------------
_SEG_STATUS = {}


def seg_label_status(device):
    """The int32 status word (on `device`) that the segmentation loss sets to 1 when it meets a label that is neither
    ignore_index nor a class number. One word per device, allocated on first use."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SEG_STATUS:
        _SEG_STATUS[key] = torch.zeros((1,), device=device, dtype=torch.int32)
    return _SEG_STATUS[key]


def seg_check_labels(device=None):
    """Read the status word back (this waits for the device), clear it, and raise when a seg_loss / seg_stats call since
    the last check met a label outside [0, C) that was not ignore_index. Such a label is left out of the loss, the counts
    and the gradient (torch's own kernel device-asserts on it); call this where a wait is affordable."""
    status = seg_label_status(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    bad = int(status.item())
    status.zero_()
    if bad:
        raise RuntimeError("seg_loss: a label lies outside [0, C) and is not ignore_index")


def _seg_operands(name, logits, labels, weight):
    """Contiguous detached operands: logits (B, C, S) float32 / float64, labels int32 / int64, weight of the logits' type."""
    if not logits.is_floating_point() or logits.dim() < 2:
        raise RuntimeError("%s: logits must be a floating (B, C, *) tensor" % name)
    if labels.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("%s: labels must be int32 or int64, got %s" % (name, labels.dtype))
    if labels.dim() != logits.dim() - 1 or labels.shape[0] != logits.shape[0] \
            or tuple(labels.shape[1:]) != tuple(logits.shape[2:]):
        raise RuntimeError("%s: logits (B, C, *) and labels (B, *) expected, got %s and %s"
                           % (name, tuple(logits.shape), tuple(labels.shape)))
    Cc = logits.shape[1]
    if Cc < 1 or Cc > 256:
        raise RuntimeError("%s: 1 to 256 classes are supported, got C = %d" % (name, Cc))
    _dev(logits, labels, weight)
    if labels.device != logits.device:
        raise RuntimeError("%s: labels on %s, logits on %s" % (name, labels.device, logits.device))
    x = logits.detach()
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    x = x.contiguous()
    if weight is not None:
        if weight.dim() != 1 or weight.numel() != Cc or not weight.is_floating_point():
            raise RuntimeError("%s: weight must be a floating tensor of C = %d elements" % (name, Cc))
        weight = weight.detach().to(x.dtype).contiguous()
    S = 1
    for d in x.shape[2:]:
        S *= int(d)
    return x, labels.detach().contiguous(), weight, int(x.shape[0]), int(Cc), S


def _seg_int_outputs(Cc, device):
    buf = torch.zeros((2 + Cc * Cc,), device=device, dtype=torch.int64)      # one fill for both
    return buf[:2], buf[2:].view(Cc, Cc)


def _seg_forward(x, labels, weight, B, Cc, S, ignore_index, with_stats, want_lse):
    f64 = x.dtype == torch.float64
    part = torch.empty((lib().mvk_seg_workspace_floats(B * S),), device=x.device, dtype=x.dtype)
    out2 = torch.empty((2,), device=x.device, dtype=x.dtype)
    lse = torch.empty((B * S,), device=x.device, dtype=x.dtype) if want_lse else None
    counts, conf = _seg_int_outputs(Cc, x.device) if with_stats else (None, None)
    fn = lib().mvk_seg_loss_fwd_f64 if f64 else lib().mvk_seg_loss_fwd
    check(fn(_p(x), B, Cc, S, _p(labels), int(labels.dtype == torch.int64), int(ignore_index), _p(weight), _p(part), _p(out2),
             _p(lse), _p(counts), _p(conf), _p(seg_label_status(x.device)), _stream()))
    return out2, lse, counts, conf


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ops_, ignore_index, with_stats):
        x, labels, weight, B, Cc, S = ops_
        out2, lse, counts, conf = _seg_forward(x, labels, weight, B, Cc, S, ignore_index, with_stats, True)
        ctx.save_for_backward(x, labels, weight, out2, lse)
        ctx.geom = (B, Cc, S, int(ignore_index), logits.dtype)
        loss = out2[0].to(logits.dtype)
        if not with_stats:
            return loss
        ctx.mark_non_differentiable(counts, conf)
        return loss, counts, conf

    @staticmethod
    def backward(ctx, g, *unused):
        x, labels, weight, out2, lse = ctx.saved_tensors
        B, Cc, S, ignore_index, dtype = ctx.geom
        g = g.to(x.dtype).contiguous()
        d = torch.empty_like(x)                                              # every element is written
        fn = lib().mvk_seg_loss_bwd_f64 if x.dtype == torch.float64 else lib().mvk_seg_loss_bwd
        check(fn(_p(x), B, Cc, S, _p(labels), int(labels.dtype == torch.int64), ignore_index, _p(weight), _p(out2), _p(lse),
                 _p(g), _p(d), _stream()))
        return d.to(dtype), None, None, None


def seg_loss(logits, labels, weight=None, ignore_index=-100, with_stats=True):
    """The MVPNet baseline's segmentation loss (mvpnet/models/loss.py: F.cross_entropy(logits, labels, weight,
    ignore_index), weighted mean over the kept points) as one autograd node over one fused launch plus the ordered finish.
    logits (B, C, *) float32 or float64 (other floating types are converted to float32), labels (B, *) int32 / int64,
    weight [C] or None. Returns the scalar loss, and with with_stats (loss, (counts, conf)): counts int64 [2] =
    (kept points whose prediction equals the label, kept points), conf int64 [C, C] with rows = label and columns =
    prediction (the first maximal class), both in HBM. A point is kept when its label is not ignore_index and lies in
    [0, C); other labels set the status word of seg_check_labels and are left out. Nothing here reads the device back.
    When no gradient is wanted (torch.no_grad(), or logits that do not require one) nothing is saved and no per-point
    log-sum-exp is written."""
    ops_ = _seg_operands("seg_loss", logits, labels, weight)
    if torch.is_grad_enabled() and logits.requires_grad:
        out = _SegLossFn.apply(logits, ops_, int(ignore_index), bool(with_stats))
        return (out[0], (out[1], out[2])) if with_stats else out
    x, labels, weight, B, Cc, S = ops_
    out2, _, counts, conf = _seg_forward(x, labels, weight, B, Cc, S, ignore_index, with_stats, False)
    loss = out2[0].to(logits.dtype)
    return (loss, (counts, conf)) if with_stats else loss


def seg_stats(logits, labels, ignore_index=-100):
    """The metrics-only form of seg_loss: (counts int64 [2], conf int64 [C, C]) in HBM from one launch that computes the
    predictions only (no exp, no loss). Same label rules, same status word, no device-to-host read."""
    x, labels, _, B, Cc, S = _seg_operands("seg_stats", logits, labels, None)
    counts, conf = _seg_int_outputs(Cc, x.device)
    fn = lib().mvk_seg_loss_fwd_f64 if x.dtype == torch.float64 else lib().mvk_seg_loss_fwd
    check(fn(_p(x), B, Cc, S, _p(labels), int(labels.dtype == torch.int64), int(ignore_index), None, None, None, None,
             _p(counts), _p(conf), _p(seg_label_status(x.device)), _stream()))
    return counts, conf


def bias_act_nhwc(x, bias, res=None, bias2=None, relu=True, out=None):
    """act(x + bias[c] (+ res (+ bias2[c]))) on a channels-last 4-D tensor (in place unless `out`): the pointwise
    tail of a convolution of the frozen 2D encoder after its BatchNorm was folded into the weights."""
    _dev(x, bias, res, bias2)
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype != torch.float32:
        raise RuntimeError("bias_act_nhwc: x must be a float32 channels-last (N,C,H,W) tensor")
    if res is not None and (res.shape != x.shape or not res.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("bias_act_nhwc: the residual must have the shape and layout of x")
    y = x if out is None else out
    check(lib().mvk_bias_act_nhwc(_p(x), _p(bias), _p(res), _p(bias2), _p(y), x.numel(), x.shape[1], int(bool(relu)),
                                  _stream()))
    return y


# --------------------------------------------------------------------------------------------
# sphere extraction + sampling potentials
# --------------------------------------------------------------------------------------------

def ball_query(points, center, radius, return_d2=False):
    """Indices (ascending, int64, HBM) of the points of `points` [N,3] f32 within `radius` of `center`
    (3 host floats), float64 membership like KDTree.query_radius (ScanNet_sphere_color.py:592-597).
    Synchronises once (the count comes back to size the result)."""
    _dev(points)
    pts = _f32c(points)
    N = pts.shape[0]
    c = _np.ascontiguousarray(_np.asarray(center, dtype=_np.float64).reshape(3))
    idx = torch.empty((max(N, 1),), device=pts.device, dtype=torch.int64)
    d2 = torch.empty((max(N, 1),), device=pts.device, dtype=torch.float64) if return_d2 else None
    cnt = torch.zeros((1,), device=pts.device, dtype=torch.int64)
    ws = _workspace("ball", lib().mvk_ball_query_workspace(N), pts.device)
    check(lib().mvk_ball_query(_p(pts), N, c.ctypes.data_as(C.c_void_p), float(radius), _p(idx), _p(d2), _p(cnt),
                               _p(ws), ws.numel(), _stream()))
    n = int(cnt.item())
    return (idx[:n], d2[:n]) if return_d2 else idx[:n]


def tukey_update(points, center, radius, potentials):
    """potentials (float64, HBM) += Tukey weights of the ball around center (ScanNet_sphere_color.py:576-582)."""
    _dev(points, potentials)
    if potentials.dtype != torch.float64 or not potentials.is_contiguous():
        raise RuntimeError("tukey_update: potentials must be a contiguous float64 tensor")
    pts = _f32c(points)
    c = _np.ascontiguousarray(_np.asarray(center, dtype=_np.float64).reshape(3))
    check(lib().mvk_tukey_update(_p(pts), pts.shape[0], c.ctypes.data_as(C.c_void_p), float(radius), _p(potentials),
                                 _stream()))
    return potentials


# --------------------------------------------------------------------------------------------
# test-time voting + frozen BatchNorm apply (csrc/vote.hip); forward only, no autograd nodes
# --------------------------------------------------------------------------------------------

def _i32c(t, what):
    if t.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("%s must be int32 or int64" % what)
    return t.contiguous() if t.dtype == torch.int32 else t.to(torch.int32).contiguous()


def vote_update_batch(votes, cloud_offsets, scores, lengths, input_inds, cloud_inds, smooth=0.95, is_logits=True,
                      points=None, r2_max=0.0, labels=None, label_values=None, col_map=None, confusion=None,
                      cloud_inds_host=None):
    """One batch's smoothed votes, in place (tester.py:160-186, trainer.py:351-378): for every row i of sphere b,
    votes[cloud_offsets[cloud_inds[b]] + input_inds[i]] = smooth * old + (1 - smooth) * p[i] in float64, with p the
    float32 softmax of scores [N,C] (is_logits) or scores itself. votes [sum of cloud sizes, C] float64 and cloud_offsets
    [n_clouds + 1] int64, both in HBM. points [N,3] with r2_max > 0: only rows with |p|^2 < r2_max vote. Spheres are applied
    in batch order; the B integers of cloud_inds are the only thing read on the host (pass cloud_inds_host to skip even
    that). labels / label_values / col_map / confusion [Ctot,Ctot] int64: also count this batch's own argmax against its
    labels (trainer.py:395-412)."""
    _dev(votes, cloud_offsets, scores, lengths, input_inds, cloud_inds, points, labels, label_values, col_map, confusion)
    if votes.dtype != torch.float64 or votes.dim() != 2 or not votes.is_contiguous():
        raise RuntimeError("vote_update_batch: votes must be a contiguous float64 [rows, C] tensor")
    if cloud_offsets.dtype != torch.int64 or cloud_offsets.dim() != 1 or cloud_offsets.shape[0] < 2:
        raise RuntimeError("vote_update_batch: cloud_offsets must be int64 [n_clouds + 1]")
    scores = _f32c(scores)
    N, Cn = scores.shape
    if Cn != votes.shape[1]:
        raise RuntimeError("vote_update_batch: scores have %d columns, the votes %d" % (Cn, votes.shape[1]))
    inds, i64 = _idx(input_inds.reshape(-1))
    if inds.shape[0] != N:
        raise RuntimeError("vote_update_batch: input_inds [N] expected")
    lens = _i32c(lengths.reshape(-1), "lengths")
    cl = _i32c(cloud_inds.reshape(-1), "cloud_inds")
    B = lens.shape[0]
    if cl.shape[0] != B:
        raise RuntimeError("vote_update_batch: lengths and cloud_inds differ in size")
    host = _np.ascontiguousarray(cl.cpu().numpy() if cloud_inds_host is None else cloud_inds_host, dtype=_np.int32).reshape(-1)
    if host.shape[0] != B:
        raise RuntimeError("vote_update_batch: cloud_inds_host [B] expected")
    if points is not None:
        points = _f32c(points)
        if points.shape != (N, 3):
            raise RuntimeError("vote_update_batch: points [N,3] expected")
    lab = l64 = None
    Ctot = 0
    if confusion is not None:
        if labels is None or label_values is None or col_map is None:
            raise RuntimeError("vote_update_batch: the confusion needs labels, label_values and col_map")
        lab, l64 = _idx(labels.reshape(-1))
        Ctot = label_values.shape[0]
        if (lab.shape[0] != N or label_values.dtype != torch.int32 or col_map.dtype != torch.int32 or
                col_map.shape[0] != Ctot or confusion.dtype != torch.int64 or tuple(confusion.shape) != (Ctot, Ctot) or
                not confusion.is_contiguous()):
            raise RuntimeError("vote_update_batch: labels [N], label_values / col_map [Ctot] int32 and a contiguous "
                               "int64 confusion [Ctot,Ctot] expected")
        label_values, col_map = label_values.contiguous(), col_map.contiguous()
    smooth = float(smooth)
    check(lib().mvk_vote_update(_p(scores), N, Cn, int(bool(is_logits)), _p(points), _p(lens), B, _p(inds), i64, _p(cl),
                                host.ctypes.data_as(C.c_void_p), cloud_offsets.shape[0] - 1, _p(cloud_offsets.contiguous()),
                                _p(votes), smooth, 1 - smooth, float(r2_max), _p(lab), int(l64 or 0),
                                _p(label_values) if confusion is not None else None,
                                _p(col_map) if confusion is not None else None, Ctot, _p(confusion), _stream()))
    return votes


def vote_predict(votes, label_values, col_map, proj=None, targets=None, confusion=None):
    """preds [Nfull] int32 (raw label values) of one cloud's votes [Nc,C] float64: first maximum over the row widened by a
    zero column per ignored label (col_map [Ctot] int32: model column or -1), through the reprojection proj [Nfull]
    (int32 / int64) when given (tester.py:223-236, :273-297). targets [Nfull] int32 raw labels: the confusion
    [Ctot,Ctot] int64 (rows = truth; truths outside label_values dropped) is accumulated into `confusion` (created when
    None) and returned next to the predictions."""
    _dev(votes, label_values, col_map, proj, targets, confusion)
    if votes.dtype != torch.float64 or votes.dim() != 2 or not votes.is_contiguous():
        raise RuntimeError("vote_predict: votes must be a contiguous float64 [Nc, C] tensor")
    Ctot = label_values.shape[0]
    if label_values.dtype != torch.int32 or col_map.dtype != torch.int32 or col_map.shape[0] != Ctot:
        raise RuntimeError("vote_predict: label_values and col_map must be int32 [Ctot]")
    p64 = 0
    if proj is not None:
        proj, p64 = _idx(proj.reshape(-1))
    Nfull = votes.shape[0] if proj is None else proj.shape[0]
    preds = torch.empty((Nfull,), device=votes.device, dtype=torch.int32)
    if targets is not None:
        if targets.dtype != torch.int32 or targets.reshape(-1).shape[0] != Nfull:
            raise RuntimeError("vote_predict: targets must be int32 [Nfull]")
        targets = targets.reshape(-1).contiguous()
        if confusion is None:
            confusion = torch.zeros((Ctot, Ctot), device=votes.device, dtype=torch.int64)
        elif confusion.dtype != torch.int64 or tuple(confusion.shape) != (Ctot, Ctot) or not confusion.is_contiguous():
            raise RuntimeError("vote_predict: confusion must be a contiguous int64 [Ctot,Ctot] tensor")
    check(lib().mvk_vote_predict(_p(votes), votes.shape[0], votes.shape[1], _p(proj), p64, Nfull,
                                 _p(label_values.contiguous()), _p(col_map.contiguous()), Ctot, _p(targets), _p(preds),
                                 _p(confusion) if targets is not None else None, _stream()))
    return preds if targets is None else (preds, confusion)


def affine_lrelu(x, scale, shift, slope=1.0, addend=None):
    """LeakyReLU_slope(x * scale[col] + shift[col] (+ addend)) for rows [R,C] in one launch: a BatchNorm with frozen
    statistics (scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale), the activation and the
    residual join after it. Forward only: raises when a gradient would be needed."""
    if torch.is_grad_enabled() and (x.requires_grad or (addend is not None and addend.requires_grad)):
        raise RuntimeError("affine_lrelu is forward only (frozen inference): call it under torch.no_grad()")
    _dev(x, scale, shift, addend)
    if x.dim() != 2 or scale.shape != (x.shape[1],) or shift.shape != scale.shape:
        raise RuntimeError("affine_lrelu: x [R,C], scale [C] and shift [C] expected")
    if addend is not None and addend.shape != x.shape:
        raise RuntimeError("affine_lrelu: the addend must have the shape of x")
    x, scale, shift = _f32c(x), _f32c(scale), _f32c(shift)
    addend = None if addend is None else _f32c(addend)
    y = torch.empty_like(x)
    check(lib().mvk_affine_lrelu(_p(x), _p(scale), _p(shift), _p(addend), x.shape[0], x.shape[1], float(slope), _p(y),
                                 _stream()))
    return y


# --------------------------------------------------------------------------------------------
# MVPNet whole-scene test: chunk boxes, logit votes, confusion (csrc/chunk.hip); forward only
# --------------------------------------------------------------------------------------------

def _boxes_dev(boxes, device):
    b = _np.ascontiguousarray(_np.asarray(boxes, dtype=_np.float64).reshape(-1, 4))
    return torch.from_numpy(b).to(device), b.shape[0]


def box_count(points, boxes):
    """counts [n] int64 (HBM): the points of `points` [N,3] f32 (HBM) inside each of the n xy boxes, `boxes` a HOST
    float64 array [n,4] (x_lo, y_lo, x_hi, y_hi). Both ends inclusive, compared in float64 (chunk_util.py:39,43). One
    launch for all boxes; nothing comes back to the host."""
    _dev(points)
    pts = _f32c(points)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("box_count: points [N,3] expected")
    bx, n = _boxes_dev(boxes, pts.device)
    counts = torch.empty((n,), device=pts.device, dtype=torch.int64)
    check(lib().mvk_box_count(_p(pts), pts.shape[0], _p(bx), n, _p(counts), _stream()))
    return counts


def box_select(points, boxes, counts_host, with_z=True):
    """The members of every box in ascending order as one CSR: (offsets [n+1] int64, idx [total] int64, zmin [n] f32,
    zmax [n] f32), all in HBM (zmin / zmax None without with_z). counts_host: the n counts that box_count gave for these
    boxes, on the HOST (the caller has read them to choose the boxes); they size the result, so nothing is read back."""
    _dev(points)
    pts = _f32c(points)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("box_select: points [N,3] expected")
    bx, n = _boxes_dev(boxes, pts.device)
    cnt = _np.asarray(counts_host, dtype=_np.int64).reshape(-1)
    if cnt.shape[0] != n or (cnt < 0).any():
        raise RuntimeError("box_select: one non-negative count per box expected")
    off_host = _np.zeros(n + 1, _np.int64)
    _np.cumsum(cnt, out=off_host[1:])
    total = int(off_host[-1])
    offsets = torch.from_numpy(off_host).to(pts.device)
    idx = torch.empty((total,), device=pts.device, dtype=torch.int64)
    zmin = torch.empty((n,), device=pts.device, dtype=torch.float32) if with_z else None
    zmax = torch.empty((n,), device=pts.device, dtype=torch.float32) if with_z else None
    ws = _workspace("box_select", lib().mvk_box_select_workspace(pts.shape[0], n), pts.device)
    check(lib().mvk_box_select(_p(pts), pts.shape[0], _p(bx), n, _p(offsets), total, _p(idx), _p(zmin), _p(zmax), _p(ws),
                               ws.numel(), _stream()))
    return offsets, idx, zmin, zmax


def _vote_state(sums, counts):
    if sums.dtype != torch.float32 or sums.dim() != 2 or not sums.is_contiguous():
        raise RuntimeError("chunk vote: sums must be a contiguous float32 [N, C] tensor")
    if counts.dtype != torch.int32 or counts.shape != (sums.shape[0],) or not counts.is_contiguous():
        raise RuntimeError("chunk vote: counts must be a contiguous int32 [N] tensor")


def chunk_vote_add(sums, counts, logits, chunk_ind):
    """One chunk's vote, in place (test_mvpnet_3d.py:164-168): sums[chunk_ind[j], c] += logits[c, j] and
    counts[chunk_ind[j]] += 1 for j < len(chunk_ind). logits [C, ld] f32 as the network returns them, ld >= len(chunk_ind):
    a padded chunk's extra columns do not vote. chunk_ind int64, distinct. sums [N,C] f32, counts [N] int32."""
    _dev(sums, counts, logits, chunk_ind)
    _vote_state(sums, counts)
    if logits.dim() != 2 or logits.shape[0] != sums.shape[1]:
        raise RuntimeError("chunk_vote_add: logits [C, ld] with C = %d expected" % sums.shape[1])
    logits = _f32c(logits)
    ind = chunk_ind.reshape(-1)
    if ind.dtype != torch.int64:
        raise RuntimeError("chunk_vote_add: chunk_ind must be int64")
    ind = ind.contiguous()
    if ind.shape[0] > logits.shape[1]:
        raise RuntimeError("chunk_vote_add: %d indices for %d logit columns" % (ind.shape[0], logits.shape[1]))
    check(lib().mvk_chunk_vote_add(_p(logits), logits.shape[0], logits.shape[1], _p(ind), ind.shape[0], _p(sums), _p(counts),
                                   sums.shape[0], _stream()))
    return sums, counts


def _labels64(labels, N, what):
    labels = labels.reshape(-1)
    if labels.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) or labels.shape[0] != N:
        raise RuntimeError("%s: %d integer labels expected" % (what, N))
    return labels.to(torch.int64).contiguous()


def _confusion_arg(confusion, Cn, device, what):
    if confusion is None:
        return torch.zeros((Cn, Cn), device=device, dtype=torch.int64)
    if confusion.dtype != torch.int64 or tuple(confusion.shape) != (Cn, Cn) or not confusion.is_contiguous():
        raise RuntimeError("%s: confusion must be a contiguous int64 [C,C] tensor" % what)
    return confusion


def chunk_vote_finish(sums, counts, labels=None, confusion=None, in_place=False):
    """End of a scene (test_mvpnet_3d.py:171-178): (pred [N] int64, mean [N,C] f32[, confusion [C,C] int64]). mean =
    sums / max(counts, 1) in float32 (written over sums with in_place), pred = first maximum, C where counts == 0. With
    labels [N] (integers) the pairs (truth, pred) with both in 0..C-1 are added to `confusion` (created when None), as
    sklearn's confusion_matrix(labels=arange(C)) counts them."""
    _dev(sums, counts, labels, confusion)
    _vote_state(sums, counts)
    N, Cn = sums.shape
    mean = sums if in_place else torch.empty_like(sums)
    pred = torch.empty((N,), device=sums.device, dtype=torch.int64)
    if labels is not None:
        labels = _labels64(labels, N, "chunk_vote_finish")
        confusion = _confusion_arg(confusion, Cn, sums.device, "chunk_vote_finish")
    elif confusion is not None:
        raise RuntimeError("chunk_vote_finish: a confusion needs labels")
    check(lib().mvk_chunk_vote_finish(_p(sums), _p(counts), N, Cn, _p(mean), _p(pred), _p(labels), _p(confusion), _stream()))
    return (pred, mean) if labels is None else (pred, mean, confusion)


def chunk_confusion(pred, labels, num_classes, confusion=None):
    """confusion [C,C] int64 (HBM) += the pairs (labels[i], pred[i]) with both in 0..C-1; rows = truth."""
    _dev(pred, labels, confusion)
    pred = _labels64(pred, pred.numel(), "chunk_confusion")
    labels = _labels64(labels, pred.shape[0], "chunk_confusion")
    confusion = _confusion_arg(confusion, int(num_classes), pred.device, "chunk_confusion")
    check(lib().mvk_chunk_confusion(_p(pred), _p(labels), pred.shape[0], int(num_classes), _p(confusion), _stream()))
    return confusion


# --------------------------------------------------------------------------------------------
# MVPNet whole-scene test: the inputs of G chunks at a time (csrc/scene_inputs.hip, include/mvkpconv_scene.h)
# --------------------------------------------------------------------------------------------

def _i64_vec(t, n, what):
    if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != n:
        raise RuntimeError("%s: an int64 vector of %d entries expected" % (what, n))
    return t.contiguous()


def overlap_pack(overlap):
    """pointwise_rgbd_overlap (nb, nf) bool / uint8 in HBM -> frame-major bit rows [nf, ceil(nb / 32)] int32: bit b % 32 of
    word b // 32 of row f is set when base point b is seen by frame f; bits past nb are zero. Once per scene."""
    _dev(overlap)
    if overlap.dim() != 2 or overlap.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("overlap_pack: a bool or uint8 (nb, nf) table expected")
    ov = overlap.contiguous()
    nb, nf = ov.shape
    packed = torch.empty((nf, (nb + 31) // 32), device=ov.device, dtype=torch.int32)
    check(lib().mvk_overlap_pack(_p(ov), nb, nf, _p(packed), _stream()))
    return packed


def chunk_select_frames(packed, nb, base_point_ind, rows, row_off, row_len, num_frames):
    """sel [G, num_frames] int32 (HBM): the greedy maximum-coverage frame choice of utils.voting.select_frames for G
    chunks in one launch. packed: ``overlap_pack`` of the scan's table of nb base points; base_point_ind [nb] int64; chunk
    g is rows[row_off[g] : row_off[g] + row_len[g]] (all int64, HBM), ASCENDING and DISTINCT as scene2chunks_legacy makes
    it. Ties go to the lower frame; frame 0 is chosen once nothing is left to cover. Nothing is read back."""
    _dev(packed, base_point_ind, rows, row_off, row_len)
    nb = int(nb)
    if packed.dtype != torch.int32 or packed.dim() != 2 or packed.shape[1] != (nb + 31) // 32 or not packed.is_contiguous():
        raise RuntimeError("chunk_select_frames: packed must be overlap_pack's contiguous int32 [nf, ceil(nb / 32)] rows")
    bpi = _i64_vec(base_point_ind, nb, "chunk_select_frames: base_point_ind")
    G = row_off.shape[0]
    rows = _i64_vec(rows, rows.shape[0], "chunk_select_frames: rows")
    row_off, row_len = _i64_vec(row_off, G, "chunk_select_frames: row_off"), _i64_vec(row_len, G, "chunk_select_frames: row_len")
    sel = torch.empty((G, int(num_frames)), device=packed.device, dtype=torch.int32)
    check(lib().mvk_chunk_select_frames(_p(packed), nb, packed.shape[0], _p(bpi), _p(rows), rows.shape[0], _p(row_off),
                                        _p(row_len), G, int(num_frames), _p(sel), _stream()))
    return sel


def chunk_unproject(sel, depth16, images, poses, cam_inv, bounds):
    """The chosen frames sel [G, nv] int32 of G chunks, unprojected as ``unproject_depth`` does it, masked and gathered in
    one launch: (keys [G, nv*h*w, 3] f64, image_xyz [G,nv,h,w,3] f32, image_mask [G,nv,h,w] bool, images [G,nv,3,h,w] f32,
    num_valid [G] int32). depth16 (nf,h,w) int16 (the bits of uint16 millimetres), images (nf,h,w,3) f32, poses (nf,4,4)
    f32 in HBM; cam_inv: the HOST float64 [3,3] inverse intrinsics; bounds [G,4] f64 in HBM (xlo, xhi, ylo, yhi): a pixel
    is valid when z_cam > 0 and it lies strictly inside them, in float64."""
    _dev(sel, depth16, images, poses, bounds)
    if sel.dtype != torch.int32 or sel.dim() != 2 or not sel.is_contiguous():
        raise RuntimeError("chunk_unproject: sel must be a contiguous int32 [G, nv] tensor")
    G, nv = sel.shape
    if depth16.dtype != torch.int16 or depth16.dim() != 3 or not depth16.is_contiguous():
        raise RuntimeError("chunk_unproject: depth must be a contiguous int16 (nf, h, w) tensor")
    nf, h, w = depth16.shape
    if images.dtype != torch.float32 or tuple(images.shape) != (nf, h, w, 3) or not images.is_contiguous():
        raise RuntimeError("chunk_unproject: images must be a contiguous float32 (nf, h, w, 3) tensor")
    if poses.dtype != torch.float32 or tuple(poses.shape) != (nf, 4, 4) or not poses.is_contiguous():
        raise RuntimeError("chunk_unproject: poses must be a contiguous float32 (nf, 4, 4) tensor")
    if bounds.dtype != torch.float64 or tuple(bounds.shape) != (G, 4) or not bounds.is_contiguous():
        raise RuntimeError("chunk_unproject: bounds must be a contiguous float64 [G, 4] tensor")
    kinv = _np.ascontiguousarray(cam_inv, dtype=_np.float64)
    if kinv.shape != (3, 3):
        raise RuntimeError("chunk_unproject: cam_inv must be a host [3, 3] array")
    dev = sel.device
    keys = torch.empty((G, nv * h * w, 3), device=dev, dtype=torch.float64)
    image_xyz = torch.empty((G, nv, h, w, 3), device=dev, dtype=torch.float32)
    image_mask = torch.empty((G, nv, h, w), device=dev, dtype=torch.bool)
    out = torch.empty((G, nv, 3, h, w), device=dev, dtype=torch.float32)
    num_valid = torch.empty((G,), device=dev, dtype=torch.int32)
    check(lib().mvk_chunk_unproject(_p(sel), G, nv, _p(depth16), _p(images), _p(poses), nf, h, w,
                                    kinv.ctypes.data_as(C.c_void_p), _p(bounds), _p(keys), _p(image_xyz), _p(image_mask),
                                    _p(out), _p(num_valid), _stream()))
    return keys, image_xyz, image_mask, out, num_valid


def chunk_knn_many(points, rows, row_off, q_off, row_len_host, keys, key_valid, k=3):
    """(queries [sum, 3] f32, knn [sum, k] int64): the points of G chunks (rows[row_off[g] : row_off[g] + row_len_host[g]]
    of points [N,3] f32) gathered behind each other at q_off (the running sum of the lengths, [G+1] int64 in HBM), and
    their exact float64 k-NN among chunk g's keys [G, nk, 3] f64 where key_valid [G, nk] (bool / uint8): ``knn_pixels``
    once per chunk from one C call. row_len_host: the G lengths on the HOST. -1 where a chunk has fewer than k valid keys."""
    _dev(points, rows, row_off, q_off, keys, key_valid)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("chunk_knn_many: points [N,3] float32 expected")
    pts = points.contiguous()
    lens = _np.ascontiguousarray(row_len_host, dtype=_np.int64).reshape(-1)
    G = lens.shape[0]
    qh = _np.zeros(G + 1, _np.int64)
    _np.cumsum(lens, out=qh[1:])
    rows = _i64_vec(rows, rows.shape[0], "chunk_knn_many: rows")
    row_off, q_off = _i64_vec(row_off, G, "chunk_knn_many: row_off"), _i64_vec(q_off, G + 1, "chunk_knn_many: q_off")
    if keys.dtype != torch.float64 or keys.dim() != 3 or keys.shape[0] != G or keys.shape[2] != 3 or not keys.is_contiguous():
        raise RuntimeError("chunk_knn_many: keys must be a contiguous float64 [G, nk, 3] tensor")
    nk = keys.shape[1]
    if key_valid.dtype not in (torch.bool, torch.uint8) or key_valid.numel() != G * nk or not key_valid.is_contiguous():
        raise RuntimeError("chunk_knn_many: key_valid must be a contiguous bool or uint8 tensor of G * nk entries")
    total = int(qh[-1])
    queries = torch.empty((total, 3), device=pts.device, dtype=torch.float32)
    knn = torch.empty((total, int(k)), device=pts.device, dtype=torch.int64)
    lp, qp = lens.ctypes.data_as(C.c_void_p), qh.ctypes.data_as(C.c_void_p)
    ws = _workspace("knn", lib().mvk_scene_inputs_workspace(lp, G, nk, int(k)), pts.device)
    check(lib().mvk_chunk_knn_many(_p(pts), pts.shape[0], _p(rows), rows.shape[0], _p(row_off), _p(q_off), lp, qp, G, _p(keys),
                                   _p(key_valid), nk, int(k), _p(queries), _p(knn), _p(ws), ws.numel(), _stream()))
    return queries, knn


def chunk_batch_rows(queries, knn, q_off, row_len, lengths, extras, extra_off, n_max):
    """(points [G, 3, n_max] f32, knn_indices [G, n_max, k] int64): the group as ``collate_chunks`` stacks it. Column j of
    chunk g is its row j for j < row_len[g], its row extras[extra_off[g] + j - row_len[g]] for j < lengths[g] (the pad of
    a sparse chunk; extras int32, may be empty) and zero behind. queries / knn / q_off as ``chunk_knn_many`` returns and
    takes them; row_len, lengths [G] and extra_off [G+1] int64, all in HBM."""
    _dev(queries, knn, q_off, row_len, lengths, extras, extra_off)
    G = row_len.shape[0]
    if queries.dtype != torch.float32 or queries.dim() != 2 or queries.shape[1] != 3 or not queries.is_contiguous():
        raise RuntimeError("chunk_batch_rows: queries must be a contiguous float32 [sum, 3] tensor")
    if knn.dtype != torch.int64 or knn.dim() != 2 or knn.shape[0] != queries.shape[0] or not knn.is_contiguous():
        raise RuntimeError("chunk_batch_rows: knn must be a contiguous int64 [sum, k] tensor")
    if extras.dtype != torch.int32 or extras.dim() != 1 or not extras.is_contiguous():
        raise RuntimeError("chunk_batch_rows: extras must be a contiguous int32 vector")
    q_off, extra_off = _i64_vec(q_off, G + 1, "chunk_batch_rows: q_off"), _i64_vec(extra_off, G + 1, "chunk_batch_rows: extra_off")
    row_len, lengths = _i64_vec(row_len, G, "chunk_batch_rows: row_len"), _i64_vec(lengths, G, "chunk_batch_rows: lengths")
    k, n_max = knn.shape[1], int(n_max)
    points_out = torch.empty((G, 3, n_max), device=queries.device, dtype=torch.float32)
    knn_out = torch.empty((G, n_max, k), device=queries.device, dtype=torch.int64)
    check(lib().mvk_chunk_batch_rows(_p(queries), _p(knn), _p(q_off), _p(row_len), _p(lengths),
                                     _p(extras) if extras.numel() else None, _p(extra_off), G, n_max, k, _p(points_out),
                                     _p(knn_out), _stream()))
    return points_out, knn_out


# --------------------------------------------------------------------------------------------
# MVPNet training batches from scenes resident in HBM (csrc/train_inputs.hip, include/mvkpconv_train.h)
# --------------------------------------------------------------------------------------------

class TrainResident(object):
    """S scenes one after another in HBM and their table, as include/mvkpconv_train.h lays them out: points [P,3] f32,
    labels [P] int64, base_point_ind [NB] int64, bits [NW] int32 (each scene's ``overlap_pack`` rows), depth16 [F,h,w]
    int16, images [F,h,w,3] f32, poses [F,4,4] f32, cam_inv [S,9] f64, all contiguous in HBM, and table: a HOST int64
    [S,8] array (point_off, num_points, base_off, num_base, frame_off, num_frames, bits_off in words, 0). The table is
    checked here -- every scene inside the buffers, behind its predecessor, with a point and a frame, num_base /
    num_frames within MVK_SCENE_MAX_BASE / MVK_SCENE_MAX_FRAMES -- and uploaded once."""

    def __init__(self, points, labels, base_point_ind, bits, depth16, images, poses, cam_inv, table):
        _dev(points, labels, base_point_ind, bits, depth16, images, poses, cam_inv)
        table = _np.ascontiguousarray(table, dtype=_np.int64)
        if table.ndim != 2 or table.shape[1] != 8:
            raise RuntimeError("TrainResident: table must be a host int64 [S, 8] array")
        S = table.shape[0]
        F = depth16.shape[0] if depth16.dim() == 3 else -1
        for name, t, dtype, shape in (("points", points, torch.float32, (points.shape[0], 3)),
                                      ("labels", labels, torch.int64, (points.shape[0],)),
                                      ("base_point_ind", base_point_ind, torch.int64, (base_point_ind.shape[0],)),
                                      ("bits", bits, torch.int32, (bits.shape[0],)),
                                      ("depth16", depth16, torch.int16, tuple(depth16.shape[:3])),
                                      ("images", images, torch.float32, tuple(depth16.shape[:3]) + (3,)),
                                      ("poses", poses, torch.float32, (F, 4, 4)),
                                      ("cam_inv", cam_inv, torch.float64, (S, 9))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("TrainResident: %s must be a contiguous %s tensor of shape %s (got %s %s)"
                                   % (name, str(dtype).replace("torch.", ""), shape, t.dtype, tuple(t.shape)))
        self.points, self.labels, self.base_point_ind, self.bits = points, labels, base_point_ind, bits
        self.depth16, self.images, self.poses, self.cam_inv = depth16, images, poses, cam_inv
        self.S, self.P, self.NB, self.NW, self.F = S, points.shape[0], base_point_ind.shape[0], bits.shape[0], F
        self.h, self.w = depth16.shape[1], depth16.shape[2]
        at = [0, 0, 0, 0]
        for s, (po, n, bo, nb, fo, nf, wo, _) in enumerate(table.tolist()):
            words = nf * ((nb + 31) // 32)
            if n < 1 or nf < 1:
                raise RuntimeError("TrainResident: scene %d has no point or no frame" % s)
            if nb < 0 or nb > SCENE_CONSTANTS["MVK_SCENE_MAX_BASE"] or nf > SCENE_CONSTANTS["MVK_SCENE_MAX_FRAMES"]:
                raise RuntimeError("TrainResident: scene %d has %d base points (<= %d) and %d frames (<= %d); there is no "
                                   "fallback" % (s, nb, SCENE_CONSTANTS["MVK_SCENE_MAX_BASE"], nf,
                                                 SCENE_CONSTANTS["MVK_SCENE_MAX_FRAMES"]))
            if po < at[0] or bo < at[1] or fo < at[2] or wo < at[3] or po + n > self.P or bo + nb > self.NB or \
                    fo + nf > self.F or wo + words > self.NW:
                raise RuntimeError("TrainResident: scene %d overlaps its predecessor or leaves the buffers" % s)
            at = [po + n, bo + nb, fo + nf, wo + words]
        self.table_host = table
        self.max_points = int(table[:, 1].max()) if S else 0
        self.max_base = int(table[:, 3].max()) if S else 0
        self.max_frames = int(table[:, 5].max()) if S else 0
        staged = torch.empty((S, 8), dtype=torch.int64, pin_memory=True)
        staged.numpy()[:] = table
        self.table = staged.to(points.device, non_blocking=True)

    def _totals(self):
        return self.P, self.NB, self.F, self.NW


def _train_items(who, res, scene_id):
    if not isinstance(res, TrainResident):
        raise RuntimeError("%s: a TrainResident expected" % who)
    _dev(scene_id)
    return _i64_vec(scene_id, scene_id.shape[0], who + ": scene_id"), scene_id.shape[0]


def _pair32(v, what):
    a = _np.asarray(v, dtype=_np.float32).reshape(-1)
    if a.shape[0] != 2:
        raise RuntimeError("%s: an (x, y) pair expected" % what)
    return float(a[0]), float(a[1])


def train_chunk_pick(res, scene_id, centers, row_off, total, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2),
                     chunk_thresh=0.3, max_points=None):
    """The random crop of ScanNet2D3DChunks.__getitem__ (scannet_2d3d.py:340-371) for B items in four launches:
    (counts [B,T,2] int32, chosen [B] int32, box [B,4] f32, rows [total] int64, row_len [B] int64), all in HBM.
    scene_id [B] int64; centers [B,T] int64, the scene-local point numbers of the T tries, drawn by the caller; row_off
    [B] int64 in HBM, the running sum of the items' num_points, and total, its end, on the host. chosen is the first try
    with a point of which at least chunk_thresh are labeled, -1 for the whole scene; box = (lo.x, lo.y, hi.x, hi.y) with
    the margin; the chunk's row holds the GLOBAL indices of its points, ascending. Nothing is read back."""
    sid, B = _train_items("train_chunk_pick", res, scene_id)
    _dev(centers, row_off)
    if centers.dtype != torch.int64 or centers.dim() != 2 or centers.shape[0] != B or not centers.is_contiguous():
        raise RuntimeError("train_chunk_pick: centers must be a contiguous int64 [B, T] tensor")
    T = centers.shape[1]
    row_off = _i64_vec(row_off, B, "train_chunk_pick: row_off")
    (sx, sy), (mx, my) = _pair32(chunk_size, "train_chunk_pick: chunk_size"), _pair32(chunk_margin, "train_chunk_pick: chunk_margin")
    max_points = res.max_points if max_points is None else int(max_points)
    dev, total = sid.device, int(total)
    tile = TRAIN_CONSTANTS["MVK_TRAIN_PICK_TILE"]
    block_counts = torch.empty((B * max(1, -(-max_points // tile)),), device=dev, dtype=torch.int32)
    counts = torch.empty((B, T, 2), device=dev, dtype=torch.int32)
    chosen = torch.empty((B,), device=dev, dtype=torch.int32)
    box = torch.empty((B, 4), device=dev, dtype=torch.float32)
    rows = torch.empty((total,), device=dev, dtype=torch.int64)
    row_len = torch.empty((B,), device=dev, dtype=torch.int64)
    check(lib().mvk_train_chunk_pick(_p(res.points), _p(res.labels), res.P, _p(res.table), res.S, res.NB, res.F, res.NW,
                                     _p(sid), _p(centers), B, T, sx, sy, mx, my, float(chunk_thresh), max_points,
                                     _p(row_off), total, _p(block_counts), _p(counts), _p(chosen), _p(box), _p(rows),
                                     _p(row_len), _stream()))
    return counts, chosen, box, rows, row_len


def train_chunk_resample(rows, row_off, row_len, seeds, nb_pts, key_bits=32):
    """(sample_rows [B,nb_pts] int64, sample_pos [B,nb_pts] int32): nb_pts entries of every row
    rows[row_off[b] : row_off[b] + row_len[b]] by the library's rule (include/mvkpconv_train.h: a hash of seeds[b] and the
    position; a row of at least nb_pts entries gives a uniformly drawn subset in ASCENDING position, a shorter one itself
    and hashed pads). sample_pos are positions in the row, sample_rows the row's entries there; -1 of an empty row.
    key_bits < 32 shortens the key so that ties occur (for tests)."""
    _dev(rows, row_off, row_len, seeds)
    B = seeds.shape[0]
    rows = _i64_vec(rows, rows.shape[0], "train_chunk_resample: rows")
    row_off, row_len = _i64_vec(row_off, B, "train_chunk_resample: row_off"), _i64_vec(row_len, B, "train_chunk_resample: row_len")
    seeds = _i64_vec(seeds, B, "train_chunk_resample: seeds")
    nb_pts = int(nb_pts)
    sample_rows = torch.empty((B, nb_pts), device=rows.device, dtype=torch.int64)
    sample_pos = torch.empty((B, nb_pts), device=rows.device, dtype=torch.int32)
    check(lib().mvk_train_chunk_resample(_p(rows), rows.shape[0], _p(row_off), _p(row_len), _p(seeds), B, nb_pts,
                                         int(key_bits), _p(sample_rows), _p(sample_pos), _stream()))
    return sample_rows, sample_pos


def train_select_frames(res, scene_id, rows, row_off, row_len, num_frames):
    """sel [B, num_frames] int32, scene-local: ``chunk_select_frames`` with item b reading the bit rows and base points of
    scene scene_id[b]. rows / row_off / row_len as ``train_chunk_pick`` returns and takes them (global indices)."""
    sid, B = _train_items("train_select_frames", res, scene_id)
    _dev(rows, row_off, row_len)
    rows = _i64_vec(rows, rows.shape[0], "train_select_frames: rows")
    row_off, row_len = _i64_vec(row_off, B, "train_select_frames: row_off"), _i64_vec(row_len, B, "train_select_frames: row_len")
    sel = torch.empty((B, int(num_frames)), device=sid.device, dtype=torch.int32)
    check(lib().mvk_train_select_frames(_p(res.bits), res.NW, _p(res.base_point_ind), res.NB, _p(res.table), res.S, res.P,
                                        res.F, _p(sid), _p(rows), rows.shape[0], _p(row_off), _p(row_len), B,
                                        int(num_frames), res.max_base, res.max_frames, _p(sel), _stream()))
    return sel


def _rot_arg(who, rot, B):
    if rot is None:
        return None
    _dev(rot)
    if rot.dtype != torch.float64 or rot.numel() != B * 9 or not rot.is_contiguous():
        raise RuntimeError("%s: rot must be a contiguous float64 [B, 9] tensor" % who)
    return rot


def train_unproject(res, sel, scene_id, box, flips=None, rot=None):
    """``chunk_unproject`` for items of different scenes: (keys [B, nv*h*w, 3] f64, image_xyz [B,nv,h,w,3] f32, image_mask
    [B,nv,h,w] bool, images [B,nv,3,h,w] f32, num_valid [B] int32). sel [B,nv] int32 scene-local frames; box [B,4] f32
    of ``train_chunk_pick`` (widened by 0.1 in float64, strict); flips [B,nv] uint8 / bool: the view mirrored left to
    right in every output; rot [B,9] f64: image_xyz rotated after its rounding to float32, keys not."""
    sid, B = _train_items("train_unproject", res, scene_id)
    _dev(sel, box, flips)
    if sel.dtype != torch.int32 or sel.dim() != 2 or sel.shape[0] != B or not sel.is_contiguous():
        raise RuntimeError("train_unproject: sel must be a contiguous int32 [B, nv] tensor")
    nv, h, w = sel.shape[1], res.h, res.w
    if box.dtype != torch.float32 or tuple(box.shape) != (B, 4) or not box.is_contiguous():
        raise RuntimeError("train_unproject: box must be a contiguous float32 [B, 4] tensor")
    if flips is not None and (flips.dtype not in (torch.uint8, torch.bool) or flips.numel() != B * nv or not flips.is_contiguous()):
        raise RuntimeError("train_unproject: flips must be a contiguous uint8 or bool [B, nv] tensor")
    rot = _rot_arg("train_unproject", rot, B)
    dev = sid.device
    keys = torch.empty((B, nv * h * w, 3), device=dev, dtype=torch.float64)
    image_xyz = torch.empty((B, nv, h, w, 3), device=dev, dtype=torch.float32)
    image_mask = torch.empty((B, nv, h, w), device=dev, dtype=torch.bool)
    out = torch.empty((B, nv, 3, h, w), device=dev, dtype=torch.float32)
    num_valid = torch.empty((B,), device=dev, dtype=torch.int32)
    check(lib().mvk_train_unproject(_p(sel), _p(sid), B, nv, _p(res.table), res.S, res.P, res.NB, res.F, res.NW,
                                    _p(res.depth16), _p(res.images), _p(res.poses), _p(res.cam_inv), h, w, _p(box),
                                    _p(flips), _p(rot), _p(keys), _p(image_xyz), _p(image_mask), _p(out), _p(num_valid),
                                    _stream()))
    return keys, image_xyz, image_mask, out, num_valid


def train_batch_rows(queries, labels, sample_rows, rot=None):
    """(points [B, 3, nb_pts] f32, seg_label [B, nb_pts] int64): queries [B*nb_pts, 3] f32 (``chunk_knn_many``'s gather of
    the sampled points) rotated by rot [B,9] f64 in float64 and rounded to float32 (None: copied), and labels [P] int64
    at sample_rows [B, nb_pts] int64 (-100 where a row is -1)."""
    _dev(queries, labels, sample_rows)
    if sample_rows.dtype != torch.int64 or sample_rows.dim() != 2 or not sample_rows.is_contiguous():
        raise RuntimeError("train_batch_rows: sample_rows must be a contiguous int64 [B, nb_pts] tensor")
    B, nb_pts = sample_rows.shape
    if queries.dtype != torch.float32 or tuple(queries.shape) != (B * nb_pts, 3) or not queries.is_contiguous():
        raise RuntimeError("train_batch_rows: queries must be a contiguous float32 [B * nb_pts, 3] tensor")
    labels = _i64_vec(labels, labels.shape[0], "train_batch_rows: labels")
    rot = _rot_arg("train_batch_rows", rot, B)
    points_out = torch.empty((B, 3, nb_pts), device=queries.device, dtype=torch.float32)
    seg_label = torch.empty((B, nb_pts), device=queries.device, dtype=torch.int64)
    check(lib().mvk_train_batch_rows(_p(queries), _p(labels), labels.shape[0], _p(sample_rows), _p(rot), B, nb_pts,
                                     _p(points_out), _p(seg_label), _stream()))
    return points_out, seg_label


# --------------------------------------------------------------------------------------------
# KPFCNN sphere batches from scenes resident in HBM (csrc/sphere_inputs.hip, include/mvkpconv_sphere.h)
# --------------------------------------------------------------------------------------------

def knn_f64_ragged(points, rows, q_off, keys, key_valid=None, k=3, return_queries=False):
    """The exact float64 k-NN of B items whose lengths exist only on the device, in a fixed number of launches: ``knn_pixels``
    on every item alone, bit for bit. points [N,3] f32; rows [cap] int64; q_off [B+1] int64 in HBM, non-decreasing: the
    query at slot s of [q_off[b], q_off[b+1]) is points[rows[s]] (zero when rows[s] lies outside [0, N)) and searches
    keys[b] ([B,nk,3] f64) where key_valid[b] ([B,nk] bool / uint8, None: all). Returns knn [cap,k] int64, the key's number
    in its item, -1 where the item has no valid key left and in the slots at or past q_off[B]; with return_queries also
    the gathered queries [cap,3] f32 (zeros past q_off[B]). Nothing is read back."""
    _dev(points, rows, q_off, keys, key_valid)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise RuntimeError("knn_f64_ragged: points must be a contiguous float32 [N, 3] tensor")
    if keys.dtype != torch.float64 or keys.dim() != 3 or keys.shape[2] != 3 or not keys.is_contiguous():
        raise RuntimeError("knn_f64_ragged: keys must be a contiguous float64 [B, nk, 3] tensor")
    B, nk, k = keys.shape[0], keys.shape[1], int(k)
    cap = rows.shape[0]
    rows, q_off = _i64_vec(rows, cap, "knn_f64_ragged: rows"), _i64_vec(q_off, B + 1, "knn_f64_ragged: q_off")
    if key_valid is not None and (key_valid.dtype not in (torch.bool, torch.uint8) or key_valid.numel() != B * nk
                                  or not key_valid.is_contiguous()):
        raise RuntimeError("knn_f64_ragged: key_valid must be a contiguous bool or uint8 tensor of B * nk entries")
    if not 1 <= k <= 8:
        raise RuntimeError("knn_f64_ragged: k=%d unsupported (1..8)" % k)
    nbytes = lib().mvk_knn_ragged_workspace(B, cap, nk, k) if B else 0
    if nbytes < 0:
        raise RuntimeError("knn_f64_ragged: B=%d items (1..%d) or cap + B * nk = %d (< 2^30) refused"
                           % (B, SPHERE_CONSTANTS["MVK_KNN_RAGGED_MAX_ITEMS"], cap + B * nk))
    dev = points.device
    knn = torch.empty((cap, k), device=dev, dtype=torch.int64)
    queries = torch.empty((cap, 3), device=dev, dtype=torch.float32) if return_queries else None
    if B == 0:
        knn.fill_(-1)
        if queries is not None:
            queries.zero_()
    else:
        ws = _workspace("knn_ragged", nbytes, dev)
        check(lib().mvk_knn_f64_ragged(_p(points), points.shape[0], _p(rows), cap, _p(q_off), B, _p(keys), _p(key_valid), nk,
                                       k, _p(knn), _p(queries), _p(ws), ws.numel(), _stream()))
    return (knn, queries) if return_queries else knn


class SphereResident(object):
    """What the sphere batches need beside a ``TrainResident`` (whose points are the dl-subsampled clouds): colors [P,3]
    f32, the coarse potential points pot_points [PP,3] f32 of all scenes back to back, potentials [PP] f64, all contiguous
    in HBM, and pots: a HOST int64 [S,2] array (pot_off, num_pot). The table is checked here -- every scene's potential
    points inside the buffer, behind its predecessor, at least one -- and uploaded once; min_potentials [S] f64 and
    argmin_potentials [S] int64 (scene-local, the first among equals) are computed from the potentials."""

    def __init__(self, res, colors, pot_points, potentials, pots):
        if not isinstance(res, TrainResident):
            raise RuntimeError("SphereResident: a TrainResident expected")
        _dev(colors, pot_points, potentials)
        pots = _np.ascontiguousarray(pots, dtype=_np.int64)
        if pots.ndim != 2 or tuple(pots.shape) != (res.S, 2):
            raise RuntimeError("SphereResident: pots must be a host int64 [S, 2] array")
        PP = pot_points.shape[0]
        for name, t, dtype, shape in (("colors", colors, torch.float32, (res.P, 3)),
                                      ("pot_points", pot_points, torch.float32, (PP, 3)),
                                      ("potentials", potentials, torch.float64, (PP,))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("SphereResident: %s must be a contiguous %s tensor of shape %s (got %s %s)"
                                   % (name, str(dtype).replace("torch.", ""), shape, t.dtype, tuple(t.shape)))
        at = 0
        for s, (off, n) in enumerate(pots.tolist()):
            if n < 1:
                raise RuntimeError("SphereResident: scene %d has no potential point" % s)
            if off < at or off + n > PP:
                raise RuntimeError("SphereResident: the potential points of scene %d overlap its predecessor's or leave "
                                   "the buffer" % s)
            at = off + n
        self.res, self.colors, self.pot_points, self.potentials = res, colors, pot_points, potentials
        self.PP, self.pots_host = PP, pots
        staged = torch.empty((res.S, 2), dtype=torch.int64, pin_memory=True)
        staged.numpy()[:] = pots
        self.pots = staged.to(colors.device, non_blocking=True)
        mins = [torch.min(potentials[off:off + n], 0) for off, n in pots.tolist()]
        self.min_potentials = torch.stack([m.values for m in mins]) if mins else potentials.new_zeros((0,))
        self.argmin_potentials = (torch.stack([m.indices for m in mins]) if mins
                                  else torch.zeros((0,), dtype=torch.int64, device=colors.device))


def _sphere_res(who, sres):
    if not isinstance(sres, SphereResident):
        raise RuntimeError("%s: a SphereResident expected" % who)
    return sres.res


def _slots(who, B_max):
    B_max = int(B_max)
    if not 0 <= B_max <= SPHERE_CONSTANTS["MVK_SPHERE_MAX_SLOTS"]:
        raise RuntimeError("%s: %d sphere slots (0..%d)" % (who, B_max, SPHERE_CONSTANTS["MVK_SPHERE_MAX_SLOTS"]))
    return B_max


def sphere_pick(sres, in_radius, batch_limit, max_spheres):
    """potential_item's picks (ScanNet_sphere_color.py:556-602, :690-694) for up to max_spheres spheres in one launch:
    (cloud_ind [B_max] int64, point_ind [B_max] int64, centers [B_max,3] f32, lengths [B_max] int32, num_spheres [1]
    int32), all in HBM; the resident potentials and their minima are updated. The loop ends behind the sphere with which
    the sum of the lengths exceeds batch_limit; slots never reached hold -1 / zeros. Nothing is read back."""
    res = _sphere_res("sphere_pick", sres)
    B_max = _slots("sphere_pick", max_spheres)
    dev = sres.colors.device
    cloud_ind = torch.empty((B_max,), device=dev, dtype=torch.int64)
    point_ind = torch.empty((B_max,), device=dev, dtype=torch.int64)
    centers = torch.empty((B_max, 3), device=dev, dtype=torch.float32)
    lengths = torch.empty((B_max,), device=dev, dtype=torch.int32)
    num_spheres = torch.zeros((1,), device=dev, dtype=torch.int32)
    check(lib().mvk_sphere_pick(_p(sres.pot_points), sres.PP, _p(sres.potentials), _p(sres.pots), _p(sres.min_potentials),
                                _p(sres.argmin_potentials), _p(res.points), res.P, _p(res.table), res.S, res.NB, res.F,
                                res.NW, float(in_radius), int(batch_limit), B_max, _p(cloud_ind), _p(point_ind),
                                _p(centers), _p(lengths), _p(num_spheres), _stream()))
    return cloud_ind, point_ind, centers, lengths, num_spheres


def _slot_args(who, cloud_ind, centers):
    _dev(cloud_ind, centers)
    B_max = _slots(who, cloud_ind.shape[0])
    cloud_ind = _i64_vec(cloud_ind, B_max, who + ": cloud_ind")
    if centers.dtype != torch.float32 or tuple(centers.shape) != (B_max, 3) or not centers.is_contiguous():
        raise RuntimeError("%s: centers must be a contiguous float32 [B_max, 3] tensor" % who)
    return cloud_ind, B_max


def sphere_members(res, cloud_ind, centers, radius, cap, status=None):
    """(rows [cap] int64, q_off [B_max+1] int64, status [1] int32): slot b's row rows[q_off[b] : q_off[b+1]] holds the
    GLOBAL indices, ascending, of the points of scene cloud_ind[b] within radius of centers[b] (``ball_query``'s float64
    test), for all slots in three launches. Rows that do not fit cap are dropped and status[0] is set to 1 (a given
    status is left as it is otherwise). A cloud_ind outside the table is an empty slot. Nothing is read back."""
    if not isinstance(res, TrainResident):
        raise RuntimeError("sphere_members: a TrainResident expected")
    cloud_ind, B_max = _slot_args("sphere_members", cloud_ind, centers)
    dev, cap = cloud_ind.device, int(cap)
    if status is None:
        status = torch.zeros((1,), device=dev, dtype=torch.int32)
    _dev(status)
    if status.dtype != torch.int32 or status.numel() < 1:
        raise RuntimeError("sphere_members: status must be an int32 tensor")
    tile = SPHERE_CONSTANTS["MVK_SPHERE_TILE"]
    block_counts = torch.empty((max(1, B_max * max(1, -(-res.max_points // tile))),), device=dev, dtype=torch.int32)
    rows = torch.empty((cap,), device=dev, dtype=torch.int64)
    q_off = torch.zeros((B_max + 1,), device=dev, dtype=torch.int64)
    check(lib().mvk_sphere_members(_p(res.points), res.P, _p(res.table), res.S, res.NB, res.F, res.NW, _p(cloud_ind),
                                   _p(centers), B_max, float(radius), res.max_points, cap, _p(block_counts), _p(rows),
                                   _p(q_off), _p(status), _stream()))
    return rows, q_off, status


def sphere_select_frames(res, cloud_ind, mask_rows, mask_off, num_frames):
    """sel [B_max, num_frames] int32, scene-local: the greedy frame choice of every slot on its own scene's bit rows, over
    the base points found in the slot's mask row (``sphere_members`` with in_radius + mask_margin). An empty slot chooses
    frame 0."""
    if not isinstance(res, TrainResident):
        raise RuntimeError("sphere_select_frames: a TrainResident expected")
    _dev(cloud_ind, mask_rows, mask_off)
    B_max = _slots("sphere_select_frames", cloud_ind.shape[0])
    cloud_ind = _i64_vec(cloud_ind, B_max, "sphere_select_frames: cloud_ind")
    mask_rows = _i64_vec(mask_rows, mask_rows.shape[0], "sphere_select_frames: mask_rows")
    mask_off = _i64_vec(mask_off, B_max + 1, "sphere_select_frames: mask_off")
    sel = torch.empty((B_max, int(num_frames)), device=cloud_ind.device, dtype=torch.int32)
    check(lib().mvk_sphere_select_frames(_p(res.bits), res.NW, _p(res.base_point_ind), res.NB, _p(res.table), res.S, res.P,
                                         res.F, _p(cloud_ind), _p(mask_rows), mask_rows.shape[0], _p(mask_off), B_max,
                                         int(num_frames), res.max_base, res.max_frames, _p(sel), _stream()))
    return sel


def sphere_unproject(res, sel, cloud_ind, flips=None):
    """``train_unproject`` for sphere slots: a sphere has no box, so the mask is depth > 0 alone -- the box handed on is
    (-FLT_MAX, FLT_MAX), which no finite pixel leaves -- and image_xyz is not rotated. Returns (keys [B_max, nv*h*w, 3]
    f64, image_xyz [B_max,nv,h,w,3] f32, image_mask [B_max,nv,h,w] bool, images [B_max,nv,3,h,w] f32, num_valid [B_max]
    int32); flips [B_max,nv] uint8 / bool mirrors a view in all of them."""
    big = float(_np.finfo(_np.float32).max)
    box = torch.tensor([-big, -big, big, big], dtype=torch.float32).repeat(sel.shape[0], 1)
    staged = torch.empty(tuple(box.shape), dtype=torch.float32, pin_memory=True).copy_(box)
    return train_unproject(res, sel, cloud_ind, staged.to(sel.device, non_blocking=True), flips=flips)


def sphere_batch_rows(sres, cloud_ind, centers, rows, q_off, R, scale, keep_color, knn, npix, noise=None):
    """The batch's rows in one launch (ScanNet_sphere_color.py:605-616, :657-670): a dict of HBM tensors over the cap
    slots of rows -- points [cap,3] f32 (centred in float64, rounded, then ((x0 R0j + x1 R1j) + x2 R2j) * scale_j +
    noise_ij in float32), world [cap,3] f32 ((float)((double)points + (double)centre); column 2 is the height feature),
    feat_aggre_points [cap,3] f32, colors [cap,3] f32 (times keep_color[b]), labels [cap] int64, input_inds [cap] int64
    (scene-local), knn_stacked [cap,k] int64 (knn + b * npix, -1 staying -1). R [B_max,9] f32, scale [B_max,3] f32,
    keep_color [B_max] f32 (0 or 1), noise [cap,3] f32 or None, all in HBM. Rows of no slot: zeros, -1 in the indices."""
    res = _sphere_res("sphere_batch_rows", sres)
    cloud_ind, B_max = _slot_args("sphere_batch_rows", cloud_ind, centers)
    _dev(rows, q_off, R, scale, keep_color, knn, noise)
    cap = rows.shape[0]
    rows, q_off = _i64_vec(rows, cap, "sphere_batch_rows: rows"), _i64_vec(q_off, B_max + 1, "sphere_batch_rows: q_off")
    for name, t, shape in (("R", R, (B_max, 9)), ("scale", scale, (B_max, 3)), ("keep_color", keep_color, (B_max,))) + \
            ((("noise", noise, (cap, 3)),) if noise is not None else ()):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("sphere_batch_rows: %s must be a contiguous float32 tensor of shape %s" % (name, shape))
    if knn.dtype != torch.int64 or knn.dim() != 2 or knn.shape[0] != cap or not knn.is_contiguous():
        raise RuntimeError("sphere_batch_rows: knn must be a contiguous int64 [cap, k] tensor")
    k, dev = knn.shape[1], rows.device
    f3 = lambda: torch.empty((cap, 3), device=dev, dtype=torch.float32)
    out = dict(points=f3(), world=f3(), feat_aggre_points=f3(), colors=f3(),
               labels=torch.empty((cap,), device=dev, dtype=torch.int64),
               knn_stacked=torch.empty((cap, k), device=dev, dtype=torch.int64),
               input_inds=torch.empty((cap,), device=dev, dtype=torch.int64))
    check(lib().mvk_sphere_batch_rows(_p(res.points), _p(sres.colors), _p(res.labels), res.P, _p(res.table), res.S, res.NB,
                                      res.F, res.NW, _p(cloud_ind), _p(centers), _p(rows), cap, _p(q_off), B_max, _p(R),
                                      _p(scale), _p(noise), _p(keep_color), _p(knn), k, int(npix), _p(out["points"]),
                                      _p(out["world"]), _p(out["feat_aggre_points"]), _p(out["colors"]), _p(out["labels"]),
                                      _p(out["knn_stacked"]), _p(out["input_inds"]), _stream()))
    return out
