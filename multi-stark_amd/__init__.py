"""multi-stark hot path on MI355X: Python host mirror of the reference's interface over the C ABI.

Names follow the reference: `System.new(config, circuits)` (src/system.rs:115), `SystemWitness.from_stage_1`
(src/system.rs:244), `System.prove_multiple_claims` (src/prover.rs:290), `Proof.to_bytes` (src/prover.rs:245).
All computation happens in `libmstark_hip.so` (hand-written gfx950 kernels behind include/mstark.h); there is no
CPU fallback: loading fails loudly if the library or a HIP device is missing.
"""
import ctypes as C
import os

import numpy as np

from . import frontend  # noqa: F401
from . import babybear  # noqa: F401  (the reference's second configuration, include/mstark_bb.h)
from .frontend import Params, bench_params, test_params, compile_circuit, system_blob, pack_claims  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmstark_hip.so")

u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
_lib = None


class MstarkError(RuntimeError):
    pass


def lib():
    """Load the HIP library (never a substitute): raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MstarkError("libmstark_hip.so is missing: run `python multi-stark_amd/build.py` (needs hipcc)")
        L = C.CDLL(LIB_PATH)
        L.ms_last_error.restype = C.c_char_p
        L.ms_kernel_name.restype = C.c_char_p
        _lib = L
    return _lib


def exported_symbols():
    """Every entry point include/mstark.h declares (used by the CPU-side ABI test)."""
    return ["ms_last_error", "ms_device_count", "ms_ctx_create", "ms_ctx_destroy", "ms_ctx_sync", "ms_ctx_sync_count", "ms_ctx_trim", "ms_ctx_set_profile_mask",
            "ms_ctx_kernel_stats", "ms_ctx_kernel_units", "ms_ctx_reset_stats", "ms_ctx_debug_fail_alloc", "ms_kernel_count", "ms_kernel_name", "ms_system_create",
            "ms_system_destroy", "ms_system_preprocessed_commit", "ms_system_circuit_info", "ms_system_circuit_kernels", "ms_witness_create", "ms_witness_create_host", "ms_claims_slice_range", "ms_witness_create_host_sliced", "ms_witness_prefetch",
            "ms_witness_create_device", "ms_witness_u32_add_bench", "ms_witness_blake3_compressions", "ms_blake3_compressions", "ms_witness_trace", "ms_witness_destroy", "ms_prove", "ms_prove_sharded", "ms_ctx_comm_progress", "ms_comm_rccl_unique_id", "ms_comm_rccl_create",
            "ms_comm_rccl_table", "ms_comm_rccl_bytes_moved", "ms_comm_rccl_destroy", "ms_comm_local_group_create", "ms_comm_local_group_abort",
            "ms_comm_local_group_destroy", "ms_comm_local_create", "ms_comm_local_table", "ms_comm_local_bytes_moved", "ms_comm_local_destroy", "ms_verify", "ms_verify_batch", "ms_dft_batch", "ms_coset_lde_batch", "ms_quotient_lde", "ms_mmcs_commit",
            "ms_mmcs_open", "ms_mmcs_destroy", "ms_mmcs_verify_batch", "ms_blake3", "ms_pcs_commit", "ms_pcs_open", "ms_pcs_verify", "ms_challenger_create",
            "ms_challenger_destroy", "ms_challenger_observe", "ms_challenger_observe_digests", "ms_challenger_sample_ext",
            "ms_challenger_sample_bits", "ms_stage2_trace", "ms_claims_accumulator",
            "ms_quotient_values", "ms_field_op", "ms_trace_destroy", "ms_trace_info", "ms_system_preprocessed_mmcs",
            "ms_witness_commit_stage1", "ms_challenger_observe_claims", "ms_witness_claims_accumulator", "ms_stage2_build",
            "ms_pcs_commit_traces", "ms_quotient", "ms_pcs_commit_ldes", "ms_witness_check", "ms_system_check_info", "ms_witness_lookup_balance",
            "ms_system_multiplicity_slot", "ms_witness_derive_multiplicities", "ms_witness_fill", "ms_fill_program_info",
            "ms_fill_scan_info", "ms_witness_argsort", "ms_sort_info", "ms_fill_peer_info", "ms_witness_claims_fill", "ms_claims_program_info",
            "ms_witness_claims"]


# ms_system_circuit_kernels / msbb_system_circuit_kernels (MS_KERNEL_* in include/mstark.h)
KERNEL_QUOTIENT, KERNEL_QUOTIENT_INLINE, KERNEL_STAGE2, KERNEL_STAGE2_GROUPED, KERNEL_STAGE2_TRACE = 0x1, 0x2, 0x4, 0x8, 0x10


def kernel_groups(flags):
    """G of a grouped stage-2 terms kernel (0 when it is not grouped)"""
    return (flags >> 8) & 0x1F


def _check(rc):
    if rc != 0:
        raise MstarkError(lib().ms_last_error().decode() or ("mstark error %d" % rc))


def _p(a):
    return a.ctypes.data_as(u64p)


def _b(a):
    return a.ctypes.data_as(u8p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


class DevMatrix(C.Structure):
    """ms_dev_matrix (include/mstark.h): one trace in device memory, strides in elements"""
    _fields_ = [("ptr", C.c_void_p), ("height", C.c_uint64), ("elem_bytes", C.c_uint32), ("row_stride", C.c_int64), ("col_stride", C.c_int64)]


def _is_torch(obj):
    return type(obj).__module__.split(".")[0] == "torch" and hasattr(obj, "data_ptr")


def _device_array(obj, what):
    """(pointer, shape, strides in elements, element size, is a torch tensor) of a torch tensor on a GPU or of any object with
    __cuda_array_interface__; MstarkError for anything that has no device pointer (numpy arrays, CPU tensors). The bits are
    taken as unsigned integers of the element's size whatever the dtype."""
    if _is_torch(obj):
        if not obj.is_cuda:
            raise MstarkError("%s: a CPU tensor has no device pointer (use System.witness)" % what)
        return int(obj.data_ptr()), tuple(int(x) for x in obj.shape), tuple(int(x) for x in obj.stride()), int(obj.element_size()), True
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        raise MstarkError("%s: %s has no device pointer (expected a torch tensor on the GPU or __cuda_array_interface__)" % (what, type(obj).__name__))
    shape = tuple(int(x) for x in cai["shape"])
    item = np.dtype(cai["typestr"]).itemsize
    strides = cai.get("strides")
    if strides is None:  # C-contiguous
        strides, acc = [], item
        for n in reversed(shape):
            strides.insert(0, acc)
            acc *= max(n, 1)
    if any(int(b) % item for b in strides):
        raise MstarkError("%s: strides are not whole elements" % what)
    return int(cai["data"][0] or 0), shape, tuple(int(b) // item for b in strides), item, False


def _device_traces(traces, n_circuits, widths_of):
    """the ms_dev_matrix array of witness_from_device (both configurations). widths_of(i) = main_width of circuit i, asked only
    once every entry has been found to be 2-D device memory. -> (array, heights, the first torch tensor seen or None). Nothing is
    kept alive: the library has finished reading the inputs when its call returns."""
    if len(traces) != n_circuits:
        raise MstarkError("expected one trace per circuit")
    desc, seen_torch = [], None
    for i, t in enumerate(traces):
        what = "trace of circuit %d" % i
        if t is None or (not _is_torch(t) and not hasattr(t, "__cuda_array_interface__") and hasattr(t, "__len__") and len(t) == 0):
            desc.append(None)
            continue
        ptr, shape, strides, item, is_torch = _device_array(t, what)
        if len(shape) != 2:
            raise MstarkError("%s: expected a 2-D matrix, got %d dimension(s)" % (what, len(shape)))
        if is_torch and seen_torch is None:
            seen_torch = t
        desc.append((ptr, shape, strides, item))
    arr = (DevMatrix * max(n_circuits, 1))()
    heights = []
    for i, d in enumerate(desc):
        if d is None or d[1][0] == 0:
            arr[i] = DevMatrix(None, 0, 1, 1, 1)
            heights.append(0)
            continue
        ptr, (h, w), (rs, cs), item = d
        width = widths_of(i)
        if w != width:
            raise MstarkError("trace of circuit %d: width %d, the circuit's main_width is %d" % (i, w, width))
        # an axis of one element has no stride to speak of
        arr[i] = DevMatrix(ptr or None, h, item, rs if h > 1 else max(w, 1), cs if w > 1 else 1)
        heights.append(h)
    return arr, heights, seen_torch


def _producer_stream(stream, torch_tensor):
    """the producer_stream argument: an integer handle or an object with .cuda_stream passes through; None = the tensor
    library's current stream when torch tensors were given (torch is imported only here), else NULL"""
    if stream is None:
        if torch_tensor is None:
            return None
        import torch

        stream = torch.cuda.current_stream(torch_tensor.device)
    handle = int(getattr(stream, "cuda_stream", stream))
    return C.c_void_p(handle) if handle else None  # (0 is the null stream, which the library's own stream follows anyway)


def device_count() -> int:
    """HIP devices visible to this process (ms_device_count; 0 without a GPU or driver)"""
    return int(lib().ms_device_count())


class Context:
    """One HIP device (ms_ctx)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib().ms_ctx_create(C.c_int32(device), C.byref(self.h))
        if rc != 0:
            raise MstarkError("cannot create a HIP context: " + lib().ms_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().ms_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().ms_ctx_sync(self.h))

    def sync_count(self):
        """host waits on this context's stream so far (ms_ctx_sync_count): a proof's count is the difference around it"""
        n = C.c_uint64()
        _check(lib().ms_ctx_sync_count(self.h, C.byref(n)))
        return int(n.value)

    def trim(self):
        _check(lib().ms_ctx_trim(self.h))

    def comm_progress(self):
        """(text of the last transport call ms_prove_sharded entered through this context, calls entered so far, still inside?) -
        readable from another thread while the proof runs"""
        buf = C.create_string_buffer(256)
        seq, fl = C.c_uint64(), C.c_int32()
        _check(lib().ms_ctx_comm_progress(self.h, buf, C.c_size_t(256), C.byref(seq), C.byref(fl)))
        return buf.value.decode(), int(seq.value), bool(fl.value)

    def debug_fail_alloc(self, nth):
        """diagnostics: the nth device allocation from now raises (0 = off)"""
        _check(lib().ms_ctx_debug_fail_alloc(self.h, C.c_int32(nth)))

    # ---- profiling
    def kernel_names(self):
        return [lib().ms_kernel_name(C.c_int32(i)).decode() for i in range(lib().ms_kernel_count())]

    def set_profile(self, names):
        all_names = self.kernel_names()
        mask = 0
        for n in names:
            mask |= 1 << all_names.index(n)
        _check(lib().ms_ctx_set_profile_mask(self.h, C.c_uint32(mask)))

    def reset_stats(self):
        _check(lib().ms_ctx_reset_stats(self.h))

    def kernel_stats(self):
        out = {}
        for i, n in enumerate(self.kernel_names()):
            launches, ms, byts = C.c_uint64(), C.c_double(), C.c_double()
            _check(lib().ms_ctx_kernel_stats(self.h, C.c_int32(i), C.byref(launches), C.byref(ms), C.byref(byts)))
            units = C.c_double()
            _check(lib().ms_ctx_kernel_units(self.h, C.c_int32(i), C.byref(units)))
            out[n] = {"launches": launches.value, "ms": ms.value, "alg_bytes": byts.value, "units": units.value}
        return out

    # ---- PCS-level entry points
    def dft_batch(self, m, inverse=False):
        m = _u64(m)
        out = np.empty_like(m)
        _check(lib().ms_dft_batch(self.h, _p(m), C.c_size_t(m.shape[0]), C.c_size_t(m.shape[1]), C.c_int32(int(inverse)), _p(out)))
        return out

    def coset_lde_batch(self, m, log_blowup):
        m = _u64(m)
        out = np.empty((m.shape[0] << log_blowup, m.shape[1]), dtype=np.uint64)
        _check(lib().ms_coset_lde_batch(self.h, _p(m), C.c_size_t(m.shape[0]), C.c_size_t(m.shape[1]), C.c_uint32(log_blowup), _p(out)))
        return out

    def quotient_lde(self, q, log_n, log_q, log_blowup):
        q = _u64(q)
        D = q.shape[1]
        out = np.empty((1 << (log_n + log_blowup), D << log_q), dtype=np.uint64)
        _check(lib().ms_quotient_lde(self.h, _p(q), C.c_uint32(log_n), C.c_uint32(log_q), C.c_uint32(log_blowup), C.c_size_t(D), _p(out)))
        return out

    def blake3(self, data: bytes) -> bytes:
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        out = np.zeros(32, dtype=np.uint8)
        _check(lib().ms_blake3(self.h, _b(buf), C.c_size_t(len(data)), _b(out)))
        return out.tobytes()

    def stage2_trace(self, mult, arg_offsets, args, beta, gamma, acc_in):
        mult, args, arg_offsets = _u64(mult), _u64(args), _u64(arg_offsets)
        h, L = mult.shape
        tr = np.zeros((h, max(L, 1) * 2), dtype=np.uint64)
        acc = np.zeros(2, dtype=np.uint64)
        _check(lib().ms_stage2_trace(self.h, C.c_size_t(h), C.c_size_t(L), _p(mult), _p(arg_offsets), _p(args), _p(_u64(beta)),
                                     _p(_u64(gamma)), _p(_u64(acc_in)), _p(tr), _p(acc)))
        return tr, (int(acc[0]), int(acc[1]))

    def claims_accumulator(self, claims_packed, beta, gamma):
        offs, data = claims_packed
        data = data if data.size else np.zeros(1, dtype=np.uint64)
        acc = np.zeros(2, dtype=np.uint64)
        _check(lib().ms_claims_accumulator(self.h, C.c_size_t(len(offs) - 1), _p(offs), _p(data), _p(_u64(beta)), _p(_u64(gamma)), _p(acc)))
        return int(acc[0]), int(acc[1])

    def field_op(self, op, a, b=None):
        a = _u64(a)
        bb = _u64(b) if b is not None else None
        out = np.empty_like(a)
        n = a.size // 2 if op >= 4 else a.size
        _check(lib().ms_field_op(self.h, C.c_int32(op), _p(a), _p(bb) if bb is not None else None, C.c_size_t(n), _p(out)))
        return out


class Mmcs:
    """ProverData of one MerkleTreeMmcs commitment (ms_mmcs)."""

    def __init__(self, ctx, mats, cap_height=0):
        self.ctx = ctx
        self.mats = [_u64(m) for m in mats]
        n = len(self.mats)
        ptrs = (u64p * n)(*[_p(m) for m in self.mats])
        hs = _u64([m.shape[0] for m in self.mats])
        ws = _u64([m.shape[1] for m in self.mats])
        maxh = int(hs.max())
        cap = np.zeros(32 * min(1 << cap_height, maxh), dtype=np.uint8)
        self.h = C.c_void_p()
        _check(lib().ms_mmcs_commit(ctx.h, C.c_size_t(n), ptrs, _p(hs), _p(ws), C.c_uint32(cap_height), _b(cap), C.byref(self.h)))
        self.cap = cap.tobytes()
        self.log_max = maxh.bit_length() - 1
        self.widths = ws

    def open(self, index):
        vals = np.zeros(int(self.widths.sum()), dtype=np.uint64)
        proof = np.zeros(32 * (self.log_max + 1), dtype=np.uint8)
        ns = C.c_size_t()
        _check(lib().ms_mmcs_open(self.h, C.c_size_t(index), _p(vals), _b(proof), C.byref(ns)))
        return vals, proof[: 32 * ns.value].tobytes()

    def verify_batch(self, indices, vals, siblings):
        """MerkleTreeMmcs::verify_batch of many openings of this commitment on the device (ms_mmcs_verify_batch): per
        opening its index, the values and the sibling bytes `open` returns. -> np.ndarray of 0 / 1"""
        hs = [m.shape[0] for m in self.mats]
        return mmcs_verify_batch(self.ctx, self.cap, len(self.cap) // 32, hs, self.widths, indices, vals, siblings)

    def __del__(self):
        if getattr(self, "h", None):
            lib().ms_mmcs_destroy(self.h)
            self.h = None


def mmcs_verify_batch(ctx, cap, cap_size, heights, widths, indices, vals, siblings):
    """ms_mmcs_verify_batch without an Mmcs: the commitment is its cap (`cap_size` digests), heights and widths.
    indices: n integers; vals: per opening the rows concatenated in matrix order; siblings: per opening its path bytes."""
    hs, ws = _u64(heights), _u64(widths)
    idx = _u64(indices)
    n = idx.size
    rw = int(ws.sum())
    cap_height = int(cap_size).bit_length() - 1
    if cap_size != 1 << cap_height or len(cap) != 32 * cap_size:
        raise MstarkError("a cap holds a power-of-two number of 32-byte digests")
    path = max(int(hs.max()).bit_length() - 1 - cap_height, 0) if hs.size else 0
    v = np.zeros(max(n * rw, 1), dtype=np.uint64)
    if n * rw:
        v[: n * rw] = np.concatenate([_u64(x).ravel() for x in vals]) if not isinstance(vals, np.ndarray) else _u64(vals).ravel()
    sib_bytes = b"".join(bytes(s) for s in siblings) if not isinstance(siblings, (bytes, bytearray, np.ndarray)) else bytes(siblings)
    if len(sib_bytes) != n * path * 32:
        raise MstarkError("expected %d sibling bytes per opening" % (path * 32))
    sib = np.frombuffer(sib_bytes + b"\0", dtype=np.uint8)
    capb = np.frombuffer(bytes(cap), dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _check(lib().ms_mmcs_verify_batch(ctx.h, C.c_size_t(hs.size), _p(hs), _p(ws), _b(capb), C.c_uint32(cap_height), C.c_size_t(n),
                                      _p(idx if n else np.zeros(1, dtype=np.uint64)), _p(v), _b(sib), _b(ok)))
    return ok[:n].copy()


class DeviceCommitment(Mmcs):
    """ProverData produced by a Level-2 call (ms_witness_commit_stage1, ms_pcs_commit_traces, ms_pcs_commit_ldes,
    ms_system_preprocessed_mmcs): the matrices never left the device."""

    def __init__(self, ctx, handle, cap: bytes, widths, log_max):
        self.ctx, self.h, self.cap = ctx, handle, cap
        self.widths = _u64(widths)
        self.log_max = log_max
        self.mats = []


class Trace:
    """A device-resident matrix handed between Level-2 calls (ms_trace): stage-2 evaluations or a quotient LDE."""

    def __init__(self, handle):
        self.h = handle

    def info(self):
        o = np.zeros(3, dtype=np.uint64)
        _check(lib().ms_trace_info(self.h, _p(o)))
        return int(o[0]), int(o[1]), int(o[2])

    def __del__(self):
        if getattr(self, "h", None):
            lib().ms_trace_destroy(self.h)
            self.h = None


def _cap_buffer(cap_height, max_height):
    return np.zeros(32 * min(1 << cap_height, max_height), dtype=np.uint8)


def pcs_commit_traces(ctx, traces, log_blowup, cap_height=0):
    """Pcs::commit (src/prover.rs:414-419) on evaluation handles; the handles are consumed"""
    infos = [t.info() for t in traces]
    maxh = max(h for h, _, _ in infos) << log_blowup
    cap = _cap_buffer(cap_height, maxh)
    hs = (C.c_void_p * len(traces))(*[t.h for t in traces])
    out = C.c_void_p()
    _check(lib().ms_pcs_commit_traces(ctx.h, C.c_uint32(log_blowup), C.c_uint32(cap_height), C.c_size_t(len(traces)), hs, _b(cap), C.byref(out)))
    return DeviceCommitment(ctx, out, cap.tobytes(), [w for _, w, _ in infos], maxh.bit_length() - 1)


def pcs_commit_ldes(ctx, ldes, cap_height=0):
    """Pcs::commit_ldes (src/prover.rs:526) on LDE handles; the commitment takes the matrices over"""
    infos = [t.info() for t in ldes]
    maxh = max(h for h, _, _ in infos)
    cap = _cap_buffer(cap_height, maxh)
    hs = (C.c_void_p * len(ldes))(*[t.h for t in ldes])
    out = C.c_void_p()
    _check(lib().ms_pcs_commit_ldes(ctx.h, C.c_uint32(cap_height), C.c_size_t(len(ldes)), hs, _b(cap), C.byref(out)))
    return DeviceCommitment(ctx, out, cap.tobytes(), [w for _, w, _ in infos], maxh.bit_length() - 1)


class PcsCommitment(Mmcs):
    """Pcs::commit (examples/pcs_example.rs:64-69): evaluations over the natural domains -> coset LDE + Merkle tree on the device."""

    def __init__(self, ctx, evals, log_blowup, cap_height=0):
        self.ctx = ctx
        self.mats = [_u64(m) for m in evals]
        n = len(self.mats)
        ptrs = (u64p * n)(*[_p(m) for m in self.mats])
        hs = _u64([m.shape[0] for m in self.mats])
        ws = _u64([m.shape[1] for m in self.mats])
        maxh = int(hs.max()) << log_blowup
        cap = np.zeros(32 * min(1 << cap_height, maxh), dtype=np.uint8)
        self.h = C.c_void_p()
        _check(lib().ms_pcs_commit(ctx.h, C.c_uint32(log_blowup), C.c_uint32(cap_height), C.c_size_t(n), ptrs, _p(hs), _p(ws), _b(cap),
                                   C.byref(self.h)))
        self.cap = cap.tobytes()
        self.log_max = maxh.bit_length() - 1
        self.widths = ws
        self.log_n = [int(h).bit_length() - 1 for h in hs]


class Challenger:
    """config.initialise_challenger() as a handle (ms_challenger): src/types.rs:28-81,118-130"""

    def __init__(self, params):
        self.h = C.c_void_p()
        _check(lib().ms_challenger_create(_p(_u64(params.words())), C.byref(self.h)))

    def observe(self, elems):
        e = np.atleast_1d(np.asarray(elems, dtype=np.uint64))  # dtype first: a tuple of words above 2^63 would pass through float64
        _check(lib().ms_challenger_observe(self.h, _p(e), C.c_size_t(e.size)))

    def observe_digests(self, cap: bytes):
        a = np.frombuffer(cap, dtype=np.uint8)
        _check(lib().ms_challenger_observe_digests(self.h, _b(a), C.c_size_t(len(cap) // 32)))

    def observe_claims(self, witness):
        """the claims of a device-resident witness, absorbed as src/prover.rs:369-373 does (hashed on the device when long)"""
        _check(lib().ms_challenger_observe_claims(self.h, witness.h))

    def sample_ext(self):
        o = np.zeros(2, dtype=np.uint64)
        _check(lib().ms_challenger_sample_ext(self.h, _p(o)))
        return int(o[0]), int(o[1])

    def sample_bits(self, bits):
        o = C.c_uint64()
        _check(lib().ms_challenger_sample_bits(self.h, C.c_uint32(bits), C.byref(o)))
        return o.value

    def __del__(self):
        if getattr(self, "h", None):
            lib().ms_challenger_destroy(self.h)
            self.h = None


def _flatten_points(per_round):
    n_points, pts = [], []
    for per_matrix in per_round:
        for plist in per_matrix:
            n_points.append(len(plist))
            for z in plist:
                pts.extend(int(x) for x in z)
    return _u64(n_points), _u64(pts if pts else [0])


def pcs_open(ctx, params, rounds, challenger):
    """Pcs::open (src/prover.rs:580). rounds: [(PcsCommitment | Mmcs, [[(c0, c1), ..] per matrix])].
    Returns (opened values flat, round -> matrix -> point -> column, 2 words each; FriProof bytes)."""
    n_points, pts = _flatten_points([per for _, per in rounds])
    handles = (C.c_void_p * len(rounds))(*[m.h for m, _ in rounds])
    total = sum(len(plist) * int(m.widths[i]) for m, per in rounds for i, plist in enumerate(per))
    opened = np.zeros(max(total, 1) * 2, dtype=np.uint64)
    cap = 1 << 22
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t()
    _check(lib().ms_pcs_open(ctx.h, _p(_u64(params.words())), C.c_size_t(len(rounds)), handles, _p(n_points), _p(pts), challenger.h, _p(opened),
                             C.c_size_t(opened.size), _b(out), C.c_size_t(cap), C.byref(n)))
    return opened[: total * 2].copy(), out[: n.value].tobytes()


def pcs_verify(params, rounds, opened, fri: bytes, challenger):
    """Pcs::verify. rounds: [(cap bytes, [(log_n, width)] per matrix, [[point, ..] per matrix])]; True = accepted"""
    caps = [np.frombuffer(c, dtype=np.uint8) for c, _, _ in rounds]
    cap_ptrs = (u8p * len(rounds))(*[_b(c) for c in caps])
    cap_sizes = _u64([len(c) // 32 for c, _, _ in rounds])
    n_mats = _u64([len(d) for _, d, _ in rounds])
    log_n = _u64([ln for _, d, _ in rounds for ln, _w in d])
    widths = _u64([w for _, d, _ in rounds for _ln, w in d])
    n_points, pts = _flatten_points([per for _, _, per in rounds])
    f = np.frombuffer(fri, dtype=np.uint8) if fri else np.zeros(1, dtype=np.uint8)
    op = _u64(opened) if len(opened) else np.zeros(1, dtype=np.uint64)
    ok = C.c_int32()
    _check(lib().ms_pcs_verify(_p(_u64(params.words())), C.c_size_t(len(rounds)), cap_ptrs, _p(cap_sizes), _p(n_mats), _p(log_n), _p(widths),
                               _p(n_points), _p(pts), _p(op), _b(f), C.c_size_t(len(fri)), challenger.h, C.byref(ok)))
    return ok.value == 1


class Proof:
    """Serialized `Proof<GoldilocksBlake3Config>` (src/prover.rs:213-254)."""

    def __init__(self, data: bytes, stage_ms=None):
        self._bytes = data
        self.stage_ms = stage_ms

    def to_bytes(self) -> bytes:
        return self._bytes

    @staticmethod
    def from_bytes(data: bytes):
        return Proof(bytes(data))


# SystemWitness.check: the challenges used when the caller gives none - fixed, non-trivial (the first hexadecimal digits of
# pi), so that a report is reproducible. They are public: a witness made to balance under exactly these passes the lookup
# part of the check; a caller who fears that passes its own.
CHECK_BETA = (0x243F6A8885A308D3, 0x13198A2E03707344)
CHECK_GAMMA = (0xA4093822299F31D0, 0x082EFA98EC4E6C89)
CHECK_CONSTRAINT, CHECK_LOOKUPS = 0x1, 0x2  # MS_CHECK_* of include/mstark.h
_NONE = (1 << 64) - 1


class CircuitCheck:
    """One circuit's part of a CheckReport (the ten words of ms_witness_check, named; with ext_d = 4 the twelve words of
    msbb_witness_check, whose accumulator has four coordinates)."""

    def __init__(self, index, words, root_counts, root_first, name=None, origins=None, ext_d=2):
        self.index, self.name, self.origins = index, name, origins
        self.height, self.failing_rows = int(words[0]), int(words[1])
        # (row, constraint root index, value) of the smallest failing row and the smallest failing root there; None = clean
        self.first_failure = None if int(words[2]) == _NONE else (int(words[2]), int(words[3]), int(words[4]))
        self.accumulator = tuple(int(x) for x in words[5:5 + ext_d])
        self.roots = int(words[5 + ext_d])
        self.kernel, self.lanes = int(words[6 + ext_d]) & 0xFF, int(words[6 + ext_d]) >> 8
        self.root_counts = root_counts  # np.uint64 per root: rows where it is non-zero
        self.root_first = root_first    # np.uint64 per root: the first such row (all-ones: none)

    def fields(self):
        """everything that is defined by the witness alone (what a model of the check reproduces)"""
        return (self.height, self.failing_rows, self.first_failure, self.accumulator, self.roots,
                [int(x) for x in self.root_counts], [int(x) for x in self.root_first])

    def _what(self, k):
        if self.origins is None or k >= len(self.origins) or not self.origins[k]:
            return "constraint root %d" % k
        o = self.origins[k]
        names = ["constraint %d" % x[1] if x[0] == "constraint" else "ext constraint %d coordinate %d" % (x[1], x[2]) for x in o]
        return "%s (root %d)" % (" = ".join(names), k)

    def lines(self):
        tag = "circuit %d%s" % (self.index, " (%s)" % self.name if self.name else "")
        out = []
        for k in np.nonzero(self.root_counts)[0]:
            k = int(k)
            s = "%s: %s non-zero on %d rows, first at row %d" % (tag, self._what(k), int(self.root_counts[k]), int(self.root_first[k]))
            if self.first_failure and self.first_failure[:2] == (int(self.root_first[k]), k):
                s += " (value 0x%016x)" % self.first_failure[2]
            out.append(s)
        return out


class CheckReport:
    """What SystemWitness.check returns: .verdict (mask of CHECK_CONSTRAINT / CHECK_LOOKUPS), .ok, .circuits[i]"""

    def __init__(self, verdict, circuits, beta, gamma, ext_d=2):
        self.verdict, self.circuits, self.beta, self.gamma = verdict, circuits, beta, gamma
        self.ok = verdict == 0
        self.final_accumulator = next((c.accumulator for c in reversed(circuits) if c.height), (0,) * ext_d)

    def __str__(self):
        if self.ok:
            return "witness satisfies the system (%d active circuits)" % sum(1 for c in self.circuits if c.height)
        out = [ln for c in self.circuits for ln in c.lines()]
        if self.verdict & CHECK_LOOKUPS:
            out.append("lookups unbalanced: the accumulator ends at (%s)" % ", ".join("0x%016x" % x for x in self.final_accumulator))
        return "\n".join(out)


LB_ENTRY_WORDS = 8  # MS_LB_ENTRY_WORDS of include/mstark.h
_P = (1 << 64) - (1 << 32) + 1


class BalanceEntry:
    """One unbalanced group of a LookupBalanceReport: .origin = (circuit or "claims", row or claim index, lookup slot) of its
    first member, .net (canonical, non-zero), .members, .args (the tuple without trailing zeros; None: it did not fit); p: the
    field's modulus (default Goldilocks), which only the text reads: a net above p / 2 is printed as negative"""

    def __init__(self, origin, net, members, args, p=None):
        self.origin, self.net, self.members, self.args, self.p = origin, net, members, args, _P if p is None else p

    def fields(self):
        return (self.origin, self.net, self.members, self.args)

    def line(self, names=None):
        c, r, j = self.origin
        net = self.net - self.p if self.net > self.p // 2 else self.net
        tup = "(?)" if self.args is None else "(%s)" % ", ".join(str(a) for a in self.args)
        if c == "claims":
            where = "claim %d" % r
        else:
            where = "circuit %d%s row %d lookup %d" % (c, " (%s)" % names[c] if names else "", r, j)
        return "%s: net %d over %d message%s, first at %s" % (tup, net, self.members, "" if self.members == 1 else "s", where)


class LookupBalanceReport:
    """What SystemWitness.lookup_balance returns: .ok, .messages, .groups, .unbalanced, .entries (BalanceEntry, ascending first
    origin, at most as many as asked for), .slot_counts[circuit][slot] and .claims_count (messages of unbalanced groups); p:
    the field's modulus (default Goldilocks; babybear.Witness.lookup_balance passes its own)"""

    def __init__(self, messages, groups, unbalanced, entries, slot_counts, claims_count, names=None, p=None):
        self.messages, self.groups, self.unbalanced, self.entries = messages, groups, unbalanced, entries
        self.slot_counts, self.claims_count, self.names, self.p = slot_counts, claims_count, names, _P if p is None else p
        self.ok = unbalanced == 0

    def fields(self):
        """everything, as plain values (what a model of the call reproduces)"""
        return (self.messages, self.groups, self.unbalanced, [e.fields() for e in self.entries], self.slot_counts, self.claims_count)

    def __str__(self):
        if self.ok:
            return "lookups balanced (%d messages in %d groups)" % (self.messages, self.groups)
        out = [e.line(self.names) for e in self.entries]
        if self.unbalanced > len(self.entries):
            out.append("... and %d more unbalanced groups (%d in all)" % (self.unbalanced - len(self.entries), self.unbalanced))
        for c, counts in enumerate(self.slot_counts):
            for j, n in enumerate(counts):
                if n:
                    out.append("circuit %d%s lookup %d: %d messages in unbalanced groups" % (c, " (%s)" % self.names[c] if self.names else "", j, n))
        if self.claims_count:
            out.append("claims: %d messages in unbalanced groups" % self.claims_count)
        return "\n".join(out)


DM_SUMMARY_WORDS = 6  # MS_DM_SUMMARY_WORDS of include/mstark.h


class MultTarget(C.Structure):
    """ms_mult_target (include/mstark.h): a provider slot of SystemWitness.derive_multiplicities"""
    _fields_ = [("circuit", C.c_uint32), ("slot", C.c_uint32)]


class MultiplicityReport:
    """What SystemWitness.derive_multiplicities returns: .demand_messages, .demand_groups, .served (groups of non-zero demand that
    found a provider), .unserved (those that found none), .duplicates (target rows that repeat an earlier target row's tuple),
    .entries (BalanceEntry of the unserved groups, ascending first origin, at most as many as asked for); .ok: nothing is unserved"""

    def __init__(self, demand_messages, demand_groups, served, unserved, duplicates, entries):
        self.demand_messages, self.demand_groups, self.served, self.unserved = demand_messages, demand_groups, served, unserved
        self.duplicates, self.entries = duplicates, entries
        self.ok = unserved == 0

    def fields(self):
        """everything, as plain values (what a model of the call reproduces)"""
        return (self.demand_messages, self.demand_groups, self.served, self.unserved, self.duplicates, [e.fields() for e in self.entries])

    def __str__(self):
        head = "%d demand messages in %d groups: %d served, %d unserved; %d duplicate target rows" % (
            self.demand_messages, self.demand_groups, self.served, self.unserved, self.duplicates)
        out = [head] + ["unserved " + e.line() for e in self.entries]
        if self.unserved > len(self.entries):
            out.append("... and %d more unserved groups" % (self.unserved - len(self.entries)))
        return "\n".join(out)


def _program_bytes(program):
    """the blob of a frontend.FillProgram, or the bytes themselves"""
    blob = getattr(program, "blob", program)
    return np.frombuffer(bytes(blob), dtype=np.uint8)


def fill_program_info(program):
    """ms_fill_program_info (host only): checks a fill program and tells how SystemWitness.fill would run it ->
    {"instructions", "slots", "lds_lanes" (0: global scratch), "assigned_columns"}"""
    a, o = _program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(lib().ms_fill_program_info(_b(a), C.c_size_t(a.size), _p(o)))
    return dict(zip(["instructions", "slots", "lds_lanes", "assigned_columns"], (int(x) for x in o)))


def fill_scan_info(program):
    """ms_fill_scan_info (host only): checks a fill program and tells its scan steps -> (scan steps, launches of the fill kernel
    (one per group of ordinary steps, one coefficient pass per scan), scans in the additive form, T = rows per scan tile)"""
    a, o = _program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(lib().ms_fill_scan_info(_b(a), C.c_size_t(a.size), _p(o)))
    return tuple(int(x) for x in o)


def fill_peer_info(program):
    """ms_fill_peer_info (host only): checks a fill program and tells the peers it declares (include/mstark.h, "PEER READS") ->
    [(circuit, trace: 0 preprocessed / 1 main, width)], empty for a program of the first or second format"""
    a, n = _program_bytes(program), C.c_size_t()
    rc = lib().ms_fill_peer_info(_b(a), C.c_size_t(a.size), None, C.c_size_t(0), C.byref(n))
    if rc != -3:  # (MS_ERR_BUFFER: the count)
        _check(rc)
        return []
    o = np.zeros(3 * n.value, dtype=np.uint64)
    _check(lib().ms_fill_peer_info(_b(a), C.c_size_t(a.size), _p(o), C.c_size_t(n.value), C.byref(n)))
    return [tuple(int(x) for x in o[3 * k:3 * k + 3]) for k in range(n.value)]


class FillReport:
    """What SystemWitness.fill returns: .rows, .steps, .instructions (executed per row), .lds_lanes (lanes per workgroup with the
    slot file in LDS; 0: the slots lay in a global scratch)"""

    def __init__(self, rows, steps, instructions, lds_lanes):
        self.rows, self.steps, self.instructions, self.lds_lanes = rows, steps, instructions, lds_lanes

    def fields(self):
        return (self.rows, self.steps, self.instructions, self.lds_lanes)

    def __str__(self):
        form = "slots in LDS at %d lanes" % self.lds_lanes if self.lds_lanes else "slots in a global scratch"
        return "%d rows x %d steps: %d instructions per row, %s" % (self.rows, self.steps, self.instructions, form)


CLAIMS_REPLACE, CLAIMS_APPEND = 0, 1  # MS_CLAIMS_* of include/mstark.h


def claims_program_info(program):
    """ms_claims_program_info (host only): checks a claim program (frontend.compile_claims, or its blob) and tells how
    SystemWitness.fill_claims would run it -> {"instructions", "slots", "lds_lanes" (0: global scratch), "width", "has_keep"}"""
    a, o = _program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(lib().ms_claims_program_info(_b(a), C.c_size_t(a.size), _p(o)))
    return {"instructions": int(o[0]), "slots": int(o[1]), "lds_lanes": int(o[2]), "width": int(o[3]) & 0xFFFFFFFF, "has_keep": bool(int(o[3]) >> 32)}


class ClaimsReport:
    """What SystemWitness.fill_claims returns: .rows (considered), .claims (emitted), .instructions (executed per row), .lds_lanes
    (lanes per workgroup with the slot file in LDS; 0: the slots lay in a global scratch)"""

    def __init__(self, rows, claims, instructions, lds_lanes):
        self.rows, self.claims, self.instructions, self.lds_lanes = rows, claims, instructions, lds_lanes

    def fields(self):
        return (self.rows, self.claims, self.instructions, self.lds_lanes)

    def __str__(self):
        form = "slots in LDS at %d lanes" % self.lds_lanes if self.lds_lanes else "slots in a global scratch"
        return "%d rows -> %d claims: %d instructions per row, %s" % (self.rows, self.claims, self.instructions, form)


SORT_PERM, SORT_RANK = 0, 1  # MS_SORT_* of include/mstark.h


def sort_info():
    """ms_sort_info (host only) -> (T = rows per tile, bits per digit, R = per-tile counts per round of the offsets step,
    largest number of key columns) of SystemWitness.argsort"""
    o = np.zeros(4, dtype=np.uint64)
    _check(lib().ms_sort_info(_p(o)))
    return tuple(int(x) for x in o)


class SortReport:
    """What SystemWitness.argsort returns: .rows, .keys (key columns), .passes (digit passes run), .skipped (digit passes in
    which all rows share one value)"""

    def __init__(self, rows, keys, passes, skipped):
        self.rows, self.keys, self.passes, self.skipped = rows, keys, passes, skipped

    def fields(self):
        return (self.rows, self.keys, self.passes, self.skipped)

    def __str__(self):
        return "%d rows by %d key column%s: %d digit passes run, %d skipped" % (self.rows, self.keys, "" if self.keys == 1 else "s", self.passes, self.skipped)


class SystemWitness:
    """Device-resident SystemWitness + claims (ms_witness). Built by `System.witness`."""

    def argsort(self, circuit, keys, dst, rank=False):
        """ms_witness_argsort: main column `dst` of `circuit` receives the stable permutation that sorts the rows by the key
        columns `keys` (primary first; cells compared as unsigned integers, ties by row index) - trace[t][dst] = the row at sorted
        position t - or, with rank=True, its inverse: trace[r][dst] = the position of row r. Made on the device; held lookup
        values follow. -> SortReport"""
        k = np.ascontiguousarray(list(keys), dtype=np.uint32)
        summary = np.zeros(4, dtype=np.uint64)
        _check(lib().ms_witness_argsort(self.system.h, self.h, C.c_size_t(circuit), k.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(k.size),
                                        C.c_uint32(dst), C.c_uint32(int(rank)), _p(summary)))  # (False / True are MS_SORT_PERM / MS_SORT_RANK)
        return SortReport(*(int(x) for x in summary))

    def fill(self, circuit, program, inputs=None, stream=None):
        """ms_witness_fill: the columns of `circuit` that `program` (frontend.compile_fill, or its blob) assigns, evaluated on the
        device for every row; held lookup values follow. inputs: None or a 2-D matrix in device memory (torch tensor or
        __cuda_array_interface__; 1, 2, 4 or 8-byte elements read as unsigned; any strides) of at most the circuit's height,
        rows beyond it read 0. stream: as for System.witness_from_device. A program with scan steps (frontend.scan) runs in the
        same call, group by group; its report sums the instructions and gives the smallest lanes figure over the launches of
        the fill kernel. A program with peer reads (frontend.Expr.peer / peer_next / peer_at and the peer_pre counterparts,
        compiled with peers=System.fill_peers()) reads the main or preprocessed traces of other circuits of this witness where
        they lie; only `circuit` is written. -> FillReport"""
        a = _program_bytes(program)
        mat, seen = None, None
        if inputs is not None:
            ptr, shape, strides, item, is_torch = _device_array(inputs, "fill inputs")
            if len(shape) != 2:
                raise MstarkError("fill inputs: expected a 2-D matrix, got %d dimension(s)" % len(shape))
            (h, w), (rs, cs) = shape, strides
            want = int(a[24:32].view("<u8")[0]) if a.size >= 48 else w  # the blob's n_inputs word (a shorter blob is refused below)
            if w != want:
                raise MstarkError("fill inputs: width %d, the program reads %d input columns" % (w, want))
            seen = inputs if is_torch else None
            mat = DevMatrix(ptr or None, h, item, rs if h > 1 else max(w, 1), cs if w > 1 else 1)
        summary = np.zeros(4, dtype=np.uint64)
        _check(lib().ms_witness_fill(self.h, C.c_size_t(circuit), _b(a), C.c_size_t(a.size), C.byref(mat) if mat is not None else None,
                                     _producer_stream(stream, seen), _p(summary)))
        return FillReport(*(int(x) for x in summary))

    def fill_claims(self, circuit, program, rows=None, inputs=None, append=False, stream=None):
        """ms_witness_claims_fill: the claims that `program` (frontend.compile_claims, or its blob) emits for rows [0, rows) of
        `circuit` (default: its whole height), one per row the program keeps, built on the device from the traces; they replace the
        witness's claims or, with append=True, follow them. inputs and stream as for fill. The traces are not touched. Pipeline
        order: fill, fill_claims, derive_multiplicities, check, prove. -> ClaimsReport"""
        a = _program_bytes(program)
        mat, seen = None, None
        if inputs is not None:
            ptr, shape, strides, item, is_torch = _device_array(inputs, "fill_claims inputs")
            if len(shape) != 2:
                raise MstarkError("fill_claims inputs: expected a 2-D matrix, got %d dimension(s)" % len(shape))
            (h, w), (rs, cs) = shape, strides
            want = int(a[24:32].view("<u8")[0]) if a.size >= 56 else w  # the blob's n_inputs word (a shorter blob is refused below)
            if w != want:
                raise MstarkError("fill_claims inputs: width %d, the program reads %d input columns" % (w, want))
            seen = inputs if is_torch else None
            mat = DevMatrix(ptr or None, h, item, rs if h > 1 else max(w, 1), cs if w > 1 else 1)
        if rows is None:
            need = C.c_size_t()
            rc = lib().ms_witness_trace(self.h, C.c_size_t(circuit), None, C.c_size_t(0), C.byref(need))
            if rc != -3:
                _check(rc)
            rows = need.value // max(self.system.circuit_info(circuit)["main_width"], 1)
        summary = np.zeros(4, dtype=np.uint64)
        _check(lib().ms_witness_claims_fill(self.system.h, self.h, C.c_size_t(circuit), _b(a), C.c_size_t(a.size), C.c_size_t(rows),
                                            C.byref(mat) if mat is not None else None, _producer_stream(stream, seen),
                                            C.c_uint32(CLAIMS_APPEND if append else CLAIMS_REPLACE), _p(summary)))
        return ClaimsReport(*(int(x) for x in summary))

    def claims(self):
        """the claims of a device-resident witness read back from the device (ms_witness_claims) -> (offsets: n_claims + 1
        uint64, data: uint64); claim i is data[offsets[i]:offsets[i + 1]]"""
        n, e = C.c_size_t(), C.c_size_t()
        rc = lib().ms_witness_claims(self.h, None, C.c_size_t(0), None, C.c_size_t(0), C.byref(n), C.byref(e))
        if rc != -3:  # (MS_ERR_BUFFER: the counts)
            _check(rc)
        offs, data = np.zeros(n.value + 1, dtype=np.uint64), np.zeros(e.value, dtype=np.uint64)
        _check(lib().ms_witness_claims(self.h, _p(offs), C.c_size_t(offs.size), _p(data), C.c_size_t(data.size), C.byref(n), C.byref(e)))
        return offs, data

    def derive_multiplicities(self, targets, entries=64):
        """ms_witness_derive_multiplicities: targets = [(circuit, lookup slot)], the provider slots whose multiplicity is one
        main-trace column (System.multiplicity_slot tells); that column is overwritten, on the device, with what the demand of
        all other messages of the witness asks of each row, and the held lookup values follow. -> MultiplicityReport with at
        most `entries` entries for demand no target row serves."""
        tg = (MultTarget * max(len(targets), 1))(*[MultTarget(int(c), int(j)) for c, j in targets])
        summary = np.zeros(DM_SUMMARY_WORDS, dtype=np.uint64)
        ent = np.zeros((max(entries, 1), LB_ENTRY_WORDS), dtype=np.uint64)
        args_cap = 64 * max(entries, 1)
        while True:  # (a second call writes the same bytes: it is only made when some tuple did not fit)
            args = np.zeros(args_cap, dtype=np.uint64)
            _check(lib().ms_witness_derive_multiplicities(self.h, tg, C.c_size_t(len(targets)), _p(summary), _p(ent), C.c_size_t(entries), _p(args),
                                                          C.c_size_t(args_cap)))
            n = int(summary[5])
            need = int(ent[:n, 5].sum())
            if need <= args_cap:
                break
            args_cap = need
        out = []
        for e in ent[:n]:
            origin = ("claims", int(e[1]), 0) if int(e[0]) == _NONE else (int(e[0]), int(e[1]), int(e[2]))
            a = None if int(e[6]) == _NONE else [int(x) for x in args[int(e[6]):int(e[6]) + int(e[5])]]
            out.append(BalanceEntry(origin, int(e[3]), int(e[4]), a))
        return MultiplicityReport(*(int(x) for x in summary[:5]), out)

    def lookup_balance(self, entries=64, names=None):
        """ms_witness_lookup_balance: every message of the witness grouped by its tuple, exactly (no challenges); the groups
        whose multiplicities do not cancel, with where they came from. -> LookupBalanceReport with at most `entries` entries.
        names (optional, per circuit): labels for the text of the report."""
        sysm = self.system
        nl = [sysm.circuit_info(i)["num_lookups"] for i in range(sysm.n_circuits)]
        total = sum(nl)
        summary, counts = np.zeros(4, dtype=np.uint64), np.zeros(total + 1, dtype=np.uint64)
        ent = np.zeros((max(entries, 1), LB_ENTRY_WORDS), dtype=np.uint64)
        args_cap = 64 * max(entries, 1)
        while True:
            args = np.zeros(args_cap, dtype=np.uint64)
            _check(lib().ms_witness_lookup_balance(self.h, _p(summary), _p(ent), C.c_size_t(entries), _p(args), C.c_size_t(args_cap), _p(counts),
                                                   C.c_size_t(total + 1)))
            n = int(summary[3])
            need = int(ent[:n, 5].sum())
            if need <= args_cap:
                break
            args_cap = need  # some tuple did not fit: the lengths are known now
        out = []
        for e in ent[:n]:
            origin = ("claims", int(e[1]), 0) if int(e[0]) == _NONE else (int(e[0]), int(e[1]), int(e[2]))
            a = None if int(e[6]) == _NONE else [int(x) for x in args[int(e[6]):int(e[6]) + int(e[5])]]
            out.append(BalanceEntry(origin, int(e[3]), int(e[4]), a))
        offs = np.cumsum([0] + nl)
        slot_counts = [[int(x) for x in counts[offs[i]:offs[i + 1]]] for i in range(sysm.n_circuits)]
        return LookupBalanceReport(int(summary[0]), int(summary[1]), int(summary[2]), out, slot_counts, int(counts[total]), names)

    def check(self, beta=None, gamma=None, names=None, origins=None):
        """ms_witness_check: every user constraint root of every active circuit on the trace domain, and the lookup balance
        under (beta, gamma) - default CHECK_BETA / CHECK_GAMMA. -> CheckReport. names / origins (optional, per circuit): labels
        and CompiledCircuit.zero_origins for the text of the report."""
        beta = CHECK_BETA if beta is None else tuple(int(x) for x in beta)
        gamma = CHECK_GAMMA if gamma is None else tuple(int(x) for x in gamma)
        sysm = self.system
        nc = sysm.n_circuits
        roots = [sysm.check_info(i)["roots"] for i in range(nc)]
        total = sum(roots)
        words = np.zeros((max(nc, 1), 10), dtype=np.uint64)
        cnt, first = np.zeros(max(total, 1), dtype=np.uint64), np.zeros(max(total, 1), dtype=np.uint64)
        verdict = C.c_uint32()
        _check(lib().ms_witness_check(self.h, _p(_u64(beta)), _p(_u64(gamma)), C.byref(verdict), _p(words), _p(cnt), _p(first), C.c_size_t(total)))
        circuits = []
        for i in range(nc):
            o = int(words[i, 9])
            circuits.append(CircuitCheck(i, words[i], cnt[o:o + roots[i]].copy(), first[o:o + roots[i]].copy(),
                                         names[i] if names else None, origins[i] if origins else None))
        return CheckReport(int(verdict.value), circuits, beta, gamma)

    def __init__(self, handle, rows, system):
        self.h = handle
        self.rows = rows  # sum of active trace heights
        self.system = system  # keeps System (and its Context) alive: device buffers return to that context's pool

    def __del__(self):
        if getattr(self, "h", None):
            lib().ms_witness_destroy(self.h)
            self.h = None

    def prefetch(self, on=True):
        """host-resident witness: every proof also uploads the inputs of the next one while it computes (ms_witness_prefetch)"""
        _check(lib().ms_witness_prefetch(self.h, C.c_int32(1 if on else 0)))

    def trace(self, circuit):
        """one stage-1 trace of a device-resident witness read back (ms_witness_trace): height x main_width, uint64"""
        need = C.c_size_t()
        rc = lib().ms_witness_trace(self.h, C.c_size_t(circuit), None, C.c_size_t(0), C.byref(need))
        if rc != -3:
            _check(rc)
        width = self.system.circuit_info(circuit)["main_width"]
        out = np.zeros((need.value // width, width), dtype=np.uint64)
        if need.value:
            _check(lib().ms_witness_trace(self.h, C.c_size_t(circuit), _p(out), C.c_size_t(out.size), C.byref(need)))
        return out

    # ---- Level 2 (include/mstark.h): the prover's steps one by one, everything staying on the device
    def commit_stage1(self, heights, widths):
        """pcs.commit of the stage-1 traces (src/prover.rs:338-350); heights / widths of the ACTIVE circuits"""
        sysm = self.system
        lb, ch = sysm.params.log_blowup, sysm.params.cap_height
        maxh = max(heights) << lb
        cap = _cap_buffer(ch, maxh)
        out = C.c_void_p()
        _check(lib().ms_witness_commit_stage1(self.h, _b(cap), C.byref(out)))
        return DeviceCommitment(sysm.ctx, out, cap.tobytes(), widths, maxh.bit_length() - 1)

    def claims_accumulator(self, beta, gamma):
        acc = np.zeros(2, dtype=np.uint64)
        _check(lib().ms_witness_claims_accumulator(self.h, _p(_u64(beta)), _p(_u64(gamma)), _p(acc)))
        return int(acc[0]), int(acc[1])

    def stage2_build(self, n_active, beta, gamma, acc_in):
        """LookupValues::stage_2_traces (src/prover.rs:400): ([accumulator after each active circuit], [Trace handles])"""
        accs = np.zeros(2 * n_active, dtype=np.uint64)
        hs = (C.c_void_p * n_active)()
        _check(lib().ms_stage2_build(self.h, _p(_u64(beta)), _p(_u64(gamma)), _p(_u64(acc_in)), _p(accs), hs))
        return [(int(accs[2 * i]), int(accs[2 * i + 1])) for i in range(n_active)], [Trace(C.c_void_p(h)) for h in hs]


class System:
    """System<GoldilocksBlake3Config> + ProverKey on one device."""

    def __init__(self, ctx, blob: bytes, n_circuits: int):
        self.ctx = ctx
        self.n_circuits = n_circuits
        self.blob = blob
        a = np.frombuffer(blob, dtype=np.uint8)
        self.h = C.c_void_p()
        _check(lib().ms_system_create(ctx.h, _b(a), C.c_size_t(len(blob)), C.byref(self.h)))

    @staticmethod
    def new(ctx, params, circuit_inputs):
        """`System::new(config, inputs)`: compiles each circuit with the front-end and commits the preprocessed traces."""
        compiled = [compile_circuit(ci) for ci in circuit_inputs]
        s = System(ctx, system_blob(params, compiled), len(compiled))
        s.params = params
        return s

    def __del__(self):
        if getattr(self, "h", None):
            lib().ms_system_destroy(self.h)
            self.h = None

    def preprocessed_commit(self):
        out = np.zeros(32 * 256, dtype=np.uint8)
        n = C.c_size_t()
        _check(lib().ms_system_preprocessed_commit(self.h, _b(out), C.c_size_t(out.size), C.byref(n)))
        return out[: 32 * n.value].tobytes() if n.value else None

    def circuit_info(self, ci):
        o = np.zeros(9, dtype=np.uint64)
        _check(lib().ms_system_circuit_info(self.h, C.c_size_t(ci), _p(o)))
        keys = ["main_width", "pre_width", "pre_height", "num_lookups", "stage2_width", "constraint_count",
                "max_constraint_degree", "quotient_degree", "args_width"]
        return dict(zip(keys, (int(x) for x in o)))

    def fill_peers(self):
        """{circuit: (main_width, preprocessed_width)} for every circuit: the peers= argument of frontend.compile_fill"""
        infos = [self.circuit_info(ci) for ci in range(self.n_circuits)]
        return {ci: (info["main_width"], info["pre_width"]) for ci, info in enumerate(infos)}

    def check_info(self, ci):
        """ms_system_check_info: what the witness check adds to circuit_info"""
        o = np.zeros(4, dtype=np.uint64)
        _check(lib().ms_system_check_info(self.h, C.c_size_t(ci), _p(o)))
        return dict(zip(["roots", "slots", "wave_steps", "lds_lanes"], (int(x) for x in o)))

    def multiplicity_slot(self, circuit, slot):
        """ms_system_multiplicity_slot: may lookup slot `slot` of `circuit` be a target of SystemWitness.derive_multiplicities?
        eligibility 0 yes / 1 its multiplicity is not one main-trace column (optionally negated) / 2 that column is read by
        another lookup expression of the circuit; column: the derived column; pull: the multiplicity is the negated column"""
        o = np.zeros(3, dtype=np.uint64)
        _check(lib().ms_system_multiplicity_slot(self.h, C.c_size_t(circuit), C.c_size_t(slot), _p(o)))
        return {"eligibility": int(o[0]), "column": int(o[1]), "pull": bool(o[2])}

    def circuit_kernels(self, ci):
        """ms_system_circuit_kernels: the mask of KERNEL_* bits of the kernels generated and compiled for circuit `ci` (0 = the
        generic interpreter kernels do all its work); the group count of a grouped stage-2 kernel is kernel_groups(flags)"""
        f = C.c_uint32()
        _check(lib().ms_system_circuit_kernels(self.h, C.c_size_t(ci), C.byref(f)))
        return int(f.value)

    def witness(self, traces, claims_packed, lookups=None, remote_heights=None):
        """`SystemWitness::from_stage_1` (lookups=None) or an explicit SystemWitness{traces, lookups}; uploads to HBM.
        remote_heights {circuit: height}: circuits another rank computes (prove_sharded): no trace here, height only."""
        remote_heights = remote_heights or {}
        trs = [_u64(t) if t is not None and len(t) else np.zeros((0, 1), dtype=np.uint64) for t in traces]
        n = self.n_circuits
        if len(trs) != n:
            raise MstarkError("expected one trace per circuit")
        tptr = (u64p * n)(*[None if i in remote_heights else _p(t) for i, t in enumerate(trs)])
        hs = _u64([remote_heights.get(i, t.shape[0]) for i, t in enumerate(trs)])
        mptr = aptr = None
        keep = []
        if lookups is not None:
            ms, as_ = [], []
            for (m, a) in lookups:
                m, a = _u64(m), _u64(a)
                keep += [m, a]
                ms.append(_p(m))
                as_.append(_p(a))
            mptr, aptr = (u64p * n)(*ms), (u64p * n)(*as_)
        offs, data = claims_packed
        data = data if data.size else np.zeros(1, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().ms_witness_create(self.h, tptr, _p(hs), mptr, aptr, C.c_size_t(len(offs) - 1), _p(offs), _p(data), C.byref(h)))
        return SystemWitness(h, int(hs.sum()), self)

    def host_witness(self, traces, claims_packed, remote_heights=None):
        """A SystemWitness that stays in HOST memory (ms_witness_create_host): every prove_multiple_claims uploads it,
        as the reference's prove() would receive it (benches/multi_stark.rs:292-296). The arrays are kept alive (and
        page-locked) by the returned object. remote_heights {circuit: height}: circuits another rank computes
        (prove_sharded): no trace here, height only."""
        remote_heights = remote_heights or {}
        trs = [_u64(t) if t is not None and len(t) else np.zeros((0, 1), dtype=np.uint64) for t in traces]
        n = self.n_circuits
        if len(trs) != n:
            raise MstarkError("expected one trace per circuit")
        tptr = (u64p * n)(*[None if i in remote_heights else _p(t) for i, t in enumerate(trs)])
        hs = _u64([remote_heights.get(i, t.shape[0]) for i, t in enumerate(trs)])
        offs, data = claims_packed
        data = data if data.size else np.zeros(1, dtype=np.uint64)
        h = C.c_void_p()
        pinned = C.c_int32(0)
        _check(lib().ms_witness_create_host(self.h, tptr, _p(hs), C.c_size_t(len(offs) - 1), _p(offs), _p(data), C.byref(pinned), C.byref(h)))
        w = SystemWitness(h, int(hs.sum()), self)
        w.keep = trs
        w.pinned = bool(pinned.value)
        return w

    def witness_from_device(self, traces, claims_packed, stream=None):
        """A SystemWitness from traces that already lie in DEVICE memory (ms_witness_create_device): nothing crosses PCIe, the
        library checks and copies them with one launch per circuit. traces: per circuit None (inactive) or a 2-D torch tensor on
        the context's device / any object with __cuda_array_interface__; shape, strides and element size (1, 2, 4 or 8 bytes,
        read as unsigned: an int64 tensor carries u64 values) come from the object, so row-major, column-major, column slices
        and row-step slices all work. claims_packed: the usual (offsets, data) numpy pair, or a pair of 1-D contiguous 64-bit
        device arrays. stream: the stream that fills the inputs - None = torch's current stream when torch tensors are given
        (no synchronisation needed), else the data must already be visible; or a hipStream_t handle as an integer. The inputs
        may be overwritten or freed as soon as the call returns."""
        arr, heights, seen = _device_traces(traces, self.n_circuits, lambda i: self.circuit_info(i)["main_width"])
        offs, data = claims_packed
        on_device = _is_torch(offs) or hasattr(offs, "__cuda_array_interface__")
        if on_device:
            po, so, sto, io, t_o = _device_array(offs, "claim offsets")
            pd, sd, std, idt, t_d = _device_array(data, "claim data")
            if len(so) != 1 or len(sd) != 1 or io != 8 or idt != 8 or (so[0] > 1 and sto[0] != 1) or (sd[0] > 1 and std[0] != 1) or so[0] < 1:
                raise MstarkError("device claims: expected two 1-D contiguous arrays of 64-bit words (offsets, data)")
            if seen is None and (t_o or t_d):
                seen = offs if t_o else data
            n_claims, poffs, pdata = so[0] - 1, C.c_void_p(po), C.c_void_p(pd or None)
        else:
            offs = _u64(offs)
            data = _u64(data) if len(data) else np.zeros(1, dtype=np.uint64)
            n_claims, poffs, pdata = len(offs) - 1, _p(offs), _p(data)
        h = C.c_void_p()
        _check(lib().ms_witness_create_device(self.h, arr, C.c_size_t(n_claims), poffs, pdata, C.c_int32(1 if on_device else 0),
                                              _producer_stream(stream, seen), C.byref(h)))
        return SystemWitness(h, int(sum(heights)), self)

    def claims_slice_range(self, heights, claim_offsets, rank, world):
        """(first element, count) of the claims' data that rank `rank` of `world` reads in a joint proof (ms_claims_slice_range)"""
        hs, offs = _u64(heights), _u64(claim_offsets)
        first, count = C.c_uint64(), C.c_uint64()
        _check(lib().ms_claims_slice_range(self.h, _p(hs), C.c_size_t(len(offs) - 1), _p(offs), C.c_int32(rank), C.c_int32(world), C.byref(first), C.byref(count)))
        return int(first.value), int(count.value)

    def host_witness_sliced(self, traces, claim_offsets, data_first, data_slice, head, remote_heights=None):
        """host_witness for a rank of a joint proof that holds only ITS part of the claims' data (ms_witness_create_host_sliced):
        all offsets, the elements [data_first, data_first + len(data_slice)) and the first min(total, 130) elements"""
        remote_heights = remote_heights or {}
        trs = [_u64(t) if t is not None and len(t) else np.zeros((0, 1), dtype=np.uint64) for t in traces]
        n = self.n_circuits
        if len(trs) != n:
            raise MstarkError("expected one trace per circuit")
        tptr = (u64p * n)(*[None if i in remote_heights else _p(t) for i, t in enumerate(trs)])
        hs = _u64([remote_heights.get(i, t.shape[0]) for i, t in enumerate(trs)])
        offs, sl, hd = _u64(claim_offsets), _u64(data_slice), _u64(head)
        sl_arg = sl if sl.size else np.zeros(1, dtype=np.uint64)
        hd_arg = hd if hd.size else np.zeros(1, dtype=np.uint64)
        h = C.c_void_p()
        pinned = C.c_int32(0)
        _check(lib().ms_witness_create_host_sliced(self.h, tptr, _p(hs), C.c_size_t(len(offs) - 1), _p(offs), C.c_uint64(data_first),
                                                   C.c_uint64(sl.size), _p(sl_arg), _p(hd_arg), C.c_size_t(hd.size), C.byref(pinned), C.byref(h)))
        w = SystemWitness(h, int(hs.sum()), self)
        w.keep = trs
        w.pinned = bool(pinned.value)
        return w

    def bench_witness_on_device(self, num_adds, a0=0xDEADBEEF, b0=0xCAFEBABE):
        """The bench workload's witness and claims generated in HBM (benches/multi_stark.rs:171-238) for [ByteTable, U32Add]."""
        h = C.c_void_p()
        _check(lib().ms_witness_u32_add_bench(self.h, C.c_size_t(num_adds), C.c_uint32(a0), C.c_uint32(b0), C.byref(h)))
        height = max(1, 1 << (num_adds - 1).bit_length())
        return SystemWitness(h, 256 + height, self)

    def blake3_witness_on_device(self, states_in):
        """`Blake3CompressionClaims::witness` generated in HBM (ms_witness_blake3_compressions) for the nine-circuit BLAKE3 system
        of blake3_circuit.py: states_in is n x 32 words, one compression per row (blake3_circuit.compression_states). The
        witness carries the claims [9, state_in, state_out]; its `states_out` is the n x 16 array of output words."""
        st = np.ascontiguousarray(states_in, dtype=np.uint32)
        if st.ndim != 2 or st.shape[1] != 32:
            raise MstarkError("states_in: expected n x 32 words")
        n = st.shape[0]
        out = np.zeros((max(n, 1), 16), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        h = C.c_void_p()
        _check(lib().ms_witness_blake3_compressions(self.h, C.c_size_t(n), st.ctypes.data_as(u32p), out.ctypes.data_as(u32p), C.byref(h)))
        H = 1 << (n - 1).bit_length()
        w = SystemWitness(h, 65536 + (2 * 512 + 5 * 64 + 1) * H, self)
        w.states_out = out[:n]
        return w

    def _out_buffer(self):
        # one output buffer per system, reused: a fresh 2 MB array per proof costs an mmap and a page fault per 4 KB touched
        cap = getattr(self, "_proof_cap", 1 << 21)
        buf = getattr(self, "_proof_buf", None)
        if buf is None or buf.size != cap:
            buf = self._proof_buf = np.zeros(cap, dtype=np.uint8)
        return buf, cap

    def prove_multiple_claims(self, witness, want_times=False):
        times = np.zeros(6, dtype=np.float64)
        while True:
            out, cap = self._out_buffer()
            n = C.c_size_t()
            rc = lib().ms_prove(self.h, witness.h, _b(out), C.c_size_t(cap), C.byref(n),
                                times.ctypes.data_as(C.POINTER(C.c_double)) if want_times else None)
            if rc == -3:
                self._proof_cap = n.value
                continue
            _check(rc)
            keys = ["stage1_commit", "lookup_construction", "stage2_commit", "quotient", "fri_open", "total"]
            return Proof(C.string_at(out.ctypes.data, n.value), dict(zip(keys, times.tolist())) if want_times else None)

    prove = prove_multiple_claims

    def verify_multiple_claims(self, claims_packed, proof) -> int:
        """`System::verify_multiple_claims`: 0 = accepted, else the VerificationError code (2 opening, 3 shape, 4 system,
        5 out-of-domain mismatch, 6 unbalanced channel). `proof`: bytes or a Proof."""
        data = proof.to_bytes() if isinstance(proof, Proof) else bytes(proof)
        buf = np.frombuffer(data, dtype=np.uint8)
        offs, cd = claims_packed
        cd = cd if cd.size else np.zeros(1, dtype=np.uint64)
        verdict = C.c_int32(-1)
        _check(lib().ms_verify(self.h, C.c_size_t(len(offs) - 1), _p(offs), _p(cd), _b(buf), C.c_size_t(len(data)), C.byref(verdict)))
        return int(verdict.value)

    verify = verify_multiple_claims

    def verify_batch(self, items):
        """ms_verify_batch: `items` is a list of (claims_packed, proof), proofs as in verify_multiple_claims. -> the list of
        verdicts verify_multiple_claims gives one by one; the per-query arithmetic and the Merkle paths of the whole batch run
        on the device."""
        n = len(items)
        if n == 0:
            _check(lib().ms_verify_batch(self.h, C.c_size_t(0), None, None, None, None, None, None))
            return []
        keep, lens, ncl = [], np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        offp, datp, prp = (u64p * n)(), (u64p * n)(), (u8p * n)()
        for i, (claims_packed, proof) in enumerate(items):
            data = proof.to_bytes() if isinstance(proof, Proof) else bytes(proof)
            buf = np.frombuffer(data + b"\0", dtype=np.uint8)  # (a zero-length proof still needs an address)
            offs, cd = claims_packed
            offs = _u64(offs)
            cd = _u64(cd) if len(cd) else np.zeros(1, dtype=np.uint64)
            keep.append((buf, offs, cd))
            lens[i], ncl[i] = len(data), len(offs) - 1
            offp[i], datp[i], prp[i] = _p(offs), _p(cd), _b(buf)
        verdicts = np.full(n, -1, dtype=np.int32)
        _check(lib().ms_verify_batch(self.h, C.c_size_t(n), _p(ncl), offp, datp, prp, _p(lens), verdicts.ctypes.data_as(C.POINTER(C.c_int32))))
        return [int(v) for v in verdicts]

    def prove_sharded(self, witness, comm, owners, want_times=False):
        """The same Proof computed by `comm.world` ranks (ms_prove_sharded; see multi-stark_amd/sharded.py for `comm`).
        owners[i] = rank computing circuit i, -1 = replicated. Collective: every rank calls it; every rank gets the bytes."""
        times = np.zeros(6, dtype=np.float64)
        own = np.ascontiguousarray(owners, dtype=np.int32)
        if own.size != self.n_circuits:
            raise MstarkError("expected one owner per circuit")
        while True:
            out, cap = self._out_buffer()
            n = C.c_size_t()
            rc = lib().ms_prove_sharded(self.h, witness.h, C.byref(comm.struct), own.ctypes.data_as(C.POINTER(C.c_int32)), _b(out),
                                        C.c_size_t(cap), C.byref(n), times.ctypes.data_as(C.POINTER(C.c_double)) if want_times else None)
            comm.reraise()
            if rc == -3:
                self._proof_cap = n.value
                continue
            _check(rc)
            keys = ["stage1_commit", "lookup_construction", "stage2_commit", "quotient", "fri_open", "total"]
            return Proof(C.string_at(out.ctypes.data, n.value), dict(zip(keys, times.tolist())) if want_times else None)

    def preprocessed_mmcs(self, heights_widths):
        """the ProverKey's preprocessed prover data as a commitment handle (None without preprocessed traces);
        heights_widths: [(lde_height, width)] of the preprocessed matrices"""
        out = C.c_void_p()
        _check(lib().ms_system_preprocessed_mmcs(self.h, C.byref(out)))
        if not out:
            return None
        maxh = max(h for h, _ in heights_widths)
        return DeviceCommitment(self.ctx, out, self.preprocessed_commit(), [w for _, w in heights_widths], maxh.bit_length() - 1)

    def quotient(self, ci, log_n, s1, s1_idx, s2, s2_idx, publics8, alpha):
        """quotient_values + shifted_quotient_slices + lde_from_shifted_coefficients (src/prover.rs:483,511-517) -> LDE handle"""
        out = C.c_void_p()
        _check(lib().ms_quotient(self.h, C.c_size_t(ci), C.c_uint32(log_n), s1.h, C.c_size_t(s1_idx), s2.h, C.c_size_t(s2_idx),
                                 _p(_u64(publics8)), _p(_u64(alpha)), C.byref(out)))
        return Trace(out)

    def quotient_values(self, ci, publics8, log_n, log_q, pre_q, s1_q, s2_q, alpha):
        N = 1 << (log_n + log_q)
        out = np.zeros((N, 2), dtype=np.uint64)
        pre = _u64(pre_q) if pre_q is not None else np.zeros(1, dtype=np.uint64)
        _check(lib().ms_quotient_values(self.h, C.c_size_t(ci), _p(_u64(publics8)), C.c_uint32(log_n), C.c_uint32(log_q), _p(pre),
                                        _p(_u64(s1_q)), _p(_u64(s2_q)), _p(_u64(alpha)), _p(out)))
        return out
