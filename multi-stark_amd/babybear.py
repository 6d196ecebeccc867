"""The reference's second configuration (BabyBear, degree-4 extension, Poseidon2, DuplexChallenger -
/root/reference/src/test_circuits/baby_bear_config.rs) over the C ABI of include/mstark_bb.h. Same interface as the
Goldilocks classes of the package: `System.new(ctx, params, circuits, poseidon2)`, `system.witness(traces, claims)`,
`system.prove_multiple_claims(witness)` -> `Proof.to_bytes()`. Elements cross the ABI as canonical u32.
All computation happens in libmstark_hip.so; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import frontend

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
P = frontend.BABYBEAR["P"]


def exported_symbols():
    """Every entry point include/mstark_bb.h declares (used by the CPU-side ABI test)."""
    return ["msbb_system_create", "msbb_system_destroy", "msbb_system_preprocessed_commit", "msbb_system_circuit_info", "msbb_system_circuit_kernels",
            "msbb_witness_create", "msbb_witness_create_host", "msbb_witness_create_device", "msbb_witness_destroy", "msbb_prove", "msbb_verify", "msbb_verify_batch", "msbb_set_poseidon2", "msbb_poseidon2_permute",
            "msbb_dft_batch", "msbb_coset_lde_batch", "msbb_mmcs_commit", "msbb_mmcs_open", "msbb_mmcs_verify_batch", "msbb_mmcs_destroy", "msbb_field_op",
            "msbb_challenger_create", "msbb_challenger_destroy", "msbb_challenger_observe", "msbb_challenger_observe_digests",
            "msbb_challenger_sample_ext", "msbb_challenger_sample_bits", "msbb_challenger_observe_claims", "msbb_trace_destroy", "msbb_trace_info",
            "msbb_system_preprocessed_mmcs", "msbb_witness_commit_stage1", "msbb_witness_claims_accumulator", "msbb_stage2_build",
            "msbb_pcs_commit_traces", "msbb_quotient", "msbb_pcs_commit_ldes", "msbb_pcs_open", "msbb_witness_check", "msbb_system_check_info",
            "msbb_witness_lookup_balance", "msbb_system_multiplicity_slot", "msbb_witness_derive_multiplicities", "msbb_witness_trace",
            "msbb_witness_fill", "msbb_fill_program_info", "msbb_fill_scan_info", "msbb_witness_argsort", "msbb_sort_info",
            "msbb_witness_claims_fill", "msbb_claims_program_info", "msbb_witness_claims"]


import sys

_PKG = sys.modules[__name__.rsplit(".", 1)[0]]  # the parent package is being imported when this module loads


def _pkg():
    return _PKG


def _lib():
    return _pkg().lib()


def _check(rc):
    if rc != 0:
        raise _pkg().MstarkError(_lib().ms_last_error().decode() or ("mstark error %d" % rc))


def _u32(a):
    a = np.asarray(a)
    if a.size and int(a.max()) >= P:
        raise _pkg().MstarkError("non-canonical BabyBear element in input")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p32(a):
    return a.ctypes.data_as(u32p)


class Proof:
    def __init__(self, data: bytes, stage_ms=None):
        self._data, self.stage_ms = data, stage_ms

    def to_bytes(self):
        return self._data


# Witness.check: the challenges used when the caller gives none - fixed, non-trivial (the first hexadecimal digits of pi, 32 bits
# at a time, reduced mod p), so that a report is reproducible. They are public: a witness made to balance under exactly these
# passes the lookup part of the check; a caller who fears that passes its own.
CHECK_BETA = tuple(x % P for x in (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344))
CHECK_GAMMA = tuple(x % P for x in (0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89))
CHECK_CIRCUIT_WORDS = 12  # MSBB_CHECK_CIRCUIT_WORDS of include/mstark_bb.h


def fill_program_info(program):
    """msbb_fill_program_info (host only): checks a fill program compiled under frontend.field(BABYBEAR) and tells how
    Witness.fill would run it -> {"instructions", "slots", "lds_lanes" (0: global scratch), "assigned_columns"}"""
    a, o = _pkg()._program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(_lib().msbb_fill_program_info(a.ctypes.data_as(u8p), C.c_size_t(a.size), o.ctypes.data_as(u64p)))
    return dict(zip(["instructions", "slots", "lds_lanes", "assigned_columns"], (int(x) for x in o)))


def fill_scan_info(program):
    """msbb_fill_scan_info (host only): checks a fill program and tells its scan steps -> (scan steps, launches of the fill kernel
    (one per group of ordinary steps, one coefficient pass per scan), scans in the additive form, T = rows per scan tile)"""
    a, o = _pkg()._program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(_lib().msbb_fill_scan_info(a.ctypes.data_as(u8p), C.c_size_t(a.size), o.ctypes.data_as(u64p)))
    return tuple(int(x) for x in o)


def compile_fill(main_width, preprocessed_width, n_inputs, steps):
    """frontend.compile_fill over this field, scan steps (frontend.scan, running_sum, running_product) included: the program
    is authored under frontend.field(BABYBEAR) - build the expressions under it too where they hold constants, which are folded
    modulo the field in force - and a program with scans comes out in the second format, "\\0MFILB02". -> frontend.FillProgram"""
    with frontend.field(frontend.BABYBEAR):
        return frontend.compile_fill(main_width, preprocessed_width, n_inputs, steps, scans=True)


def compile_claims(main_width, preprocessed_width, n_inputs, elements, keep=None):
    """frontend.compile_claims over this field: the program is authored under frontend.field(BABYBEAR) - build the expressions
    under it too where they hold constants, which are folded modulo the field in force - and comes out under the magic
    "\\0MCLAIB1". -> frontend.ClaimProgram"""
    with frontend.field(frontend.BABYBEAR):
        return frontend.compile_claims(main_width, preprocessed_width, n_inputs, elements, keep=keep)


def claims_program_info(program):
    """msbb_claims_program_info (host only): checks a claim program (babybear.compile_claims, or its blob) and tells how
    Witness.fill_claims would run it -> {"instructions", "slots", "lds_lanes" (0: global scratch), "width", "has_keep"}"""
    a, o = _pkg()._program_bytes(program), np.zeros(4, dtype=np.uint64)
    _check(_lib().msbb_claims_program_info(a.ctypes.data_as(u8p), C.c_size_t(a.size), o.ctypes.data_as(u64p)))
    return {"instructions": int(o[0]), "slots": int(o[1]), "lds_lanes": int(o[2]), "width": int(o[3]) & 0xFFFFFFFF, "has_keep": bool(int(o[3]) >> 32)}


def sort_info():
    """msbb_sort_info (host only) -> (T = rows per tile, bits per digit, R = per-tile counts per round of the offsets step,
    largest number of key columns) of Witness.argsort"""
    o = np.zeros(4, dtype=np.uint64)
    _check(_lib().msbb_sort_info(o.ctypes.data_as(u64p)))
    return tuple(int(x) for x in o)


class Witness:
    def argsort(self, circuit, keys, dst, rank=False):
        """msbb_witness_argsort: main column `dst` of `circuit` receives the stable permutation that sorts the rows by the key
        columns `keys` (primary first; cells compared as canonical values, ties by row index) - trace[t][dst] = the row at sorted
        position t - or, with rank=True, its inverse: trace[r][dst] = the position of row r. Made on the device. -> the
        package's SortReport (four digit passes per key column, run or skipped)"""
        k = np.ascontiguousarray(list(keys), dtype=np.uint32)
        summary = np.zeros(4, dtype=np.uint64)
        _check(_lib().msbb_witness_argsort(self.h, C.c_size_t(circuit), _p32(k), C.c_size_t(k.size), C.c_uint32(dst), C.c_uint32(int(rank)),
                                           summary.ctypes.data_as(u64p)))  # (False / True are MS_SORT_PERM / MS_SORT_RANK)
        return _pkg().SortReport(*(int(x) for x in summary))

    def fill(self, circuit, program, inputs=None, stream=None):
        """msbb_witness_fill: the columns of `circuit` that `program` (babybear.compile_fill, or its blob; scan steps included)
        assigns, evaluated on the device for every row. inputs: None or a 2-D matrix in device memory (torch tensor or
        __cuda_array_interface__; 1, 2 or 4-byte elements read as unsigned canonical values; any strides) of at most the
        circuit's height, rows beyond it read 0. stream: as for System.witness_from_device. -> the package's FillReport"""
        pkg = _pkg()
        a = pkg._program_bytes(program)
        mat, seen = None, None
        if inputs is not None:
            ptr, shape, strides, item, is_torch = pkg._device_array(inputs, "fill inputs")
            if len(shape) != 2:
                raise pkg.MstarkError("fill inputs: expected a 2-D matrix, got %d dimension(s)" % len(shape))
            (h, w), (rs, cs) = shape, strides
            want = int(a[24:32].view("<u8")[0]) if a.size >= 48 else w  # the blob's n_inputs word (a shorter blob is refused below)
            if w != want:
                raise pkg.MstarkError("fill inputs: width %d, the program reads %d input columns" % (w, want))
            seen = inputs if is_torch else None
            mat = pkg.DevMatrix(ptr or None, h, item, rs if h > 1 else max(w, 1), cs if w > 1 else 1)
        summary = np.zeros(4, dtype=np.uint64)
        _check(_lib().msbb_witness_fill(self.h, C.c_size_t(circuit), a.ctypes.data_as(u8p), C.c_size_t(a.size),
                                        C.byref(mat) if mat is not None else None, pkg._producer_stream(stream, seen), summary.ctypes.data_as(u64p)))
        return pkg.FillReport(*(int(x) for x in summary))

    def fill_claims(self, circuit, program, rows=None, inputs=None, append=False, stream=None):
        """msbb_witness_claims_fill: the claims that `program` (babybear.compile_claims, or its blob) emits for rows [0, rows) of
        `circuit` (default: its whole height), one per row the program keeps, built on the device from the traces; they replace the
        witness's claims or, with append=True, follow them. inputs (1, 2 or 4-byte elements) and stream as for fill. The traces
        are not touched. Pipeline order: fill, fill_claims, derive_multiplicities, check, prove. -> the package's ClaimsReport"""
        pkg = _pkg()
        a = pkg._program_bytes(program)
        mat, seen = None, None
        if inputs is not None:
            ptr, shape, strides, item, is_torch = pkg._device_array(inputs, "fill_claims inputs")
            if len(shape) != 2:
                raise pkg.MstarkError("fill_claims inputs: expected a 2-D matrix, got %d dimension(s)" % len(shape))
            (h, w), (rs, cs) = shape, strides
            want = int(a[24:32].view("<u8")[0]) if a.size >= 56 else w  # the blob's n_inputs word (a shorter blob is refused below)
            if w != want:
                raise pkg.MstarkError("fill_claims inputs: width %d, the program reads %d input columns" % (w, want))
            seen = inputs if is_torch else None
            mat = pkg.DevMatrix(ptr or None, h, item, rs if h > 1 else max(w, 1), cs if w > 1 else 1)
        if rows is None:
            need = C.c_size_t()
            rc = _lib().msbb_witness_trace(self.h, C.c_size_t(circuit), None, C.c_size_t(0), C.byref(need))
            if rc != -3:
                _check(rc)
            rows = need.value // max(self.system.circuit_info(circuit)["main_width"], 1)
        summary = np.zeros(4, dtype=np.uint64)
        _check(_lib().msbb_witness_claims_fill(self.h, C.c_size_t(circuit), a.ctypes.data_as(u8p), C.c_size_t(a.size), C.c_size_t(rows),
                                               C.byref(mat) if mat is not None else None, pkg._producer_stream(stream, seen),
                                               C.c_uint32(pkg.CLAIMS_APPEND if append else pkg.CLAIMS_REPLACE), summary.ctypes.data_as(u64p)))
        return pkg.ClaimsReport(*(int(x) for x in summary))

    def claims(self):
        """the claims of a device-resident witness read back from the device (msbb_witness_claims) -> (offsets: n_claims + 1
        uint64, data: uint32, canonical); claim i is data[offsets[i]:offsets[i + 1]]"""
        n, e = C.c_size_t(), C.c_size_t()
        rc = _lib().msbb_witness_claims(self.h, None, C.c_size_t(0), None, C.c_size_t(0), C.byref(n), C.byref(e))
        if rc != -3:  # (MS_ERR_BUFFER: the counts)
            _check(rc)
        offs, data = np.zeros(n.value + 1, dtype=np.uint64), np.zeros(e.value, dtype=np.uint32)
        _check(_lib().msbb_witness_claims(self.h, offs.ctypes.data_as(u64p), C.c_size_t(offs.size), _p32(data), C.c_size_t(data.size), C.byref(n),
                                          C.byref(e)))
        return offs, data

    def check(self, beta=None, gamma=None, names=None, origins=None):
        """msbb_witness_check: every user constraint root of every active circuit on the trace domain, and the lookup balance
        under (beta, gamma) - four canonical coordinates each, default CHECK_BETA / CHECK_GAMMA. -> the package's CheckReport
        with four-coordinate accumulators. names / origins (optional, per circuit): labels and CompiledCircuit.zero_origins for
        the text of the report."""
        pkg = _pkg()
        beta = CHECK_BETA if beta is None else tuple(int(x) for x in beta)
        gamma = CHECK_GAMMA if gamma is None else tuple(int(x) for x in gamma)
        sysm = self.system
        nc = sysm.n_circuits
        roots = [sysm.check_info(i)["roots"] for i in range(nc)]
        total = sum(roots)
        words = np.zeros((max(nc, 1), CHECK_CIRCUIT_WORDS), dtype=np.uint64)
        cnt, first = np.zeros(max(total, 1), dtype=np.uint64), np.zeros(max(total, 1), dtype=np.uint64)
        verdict = C.c_uint32()
        b, g = _raw32(beta), _raw32(gamma)  # (a coordinate >= p is the entry point's to refuse)
        if b.size != 4 or g.size != 4:
            raise pkg.MstarkError("beta and gamma have four coordinates each")
        _check(_lib().msbb_witness_check(self.h, _p32(b), _p32(g), C.byref(verdict), words.ctypes.data_as(u64p), cnt.ctypes.data_as(u64p),
                                         first.ctypes.data_as(u64p), C.c_size_t(total)))
        circuits = []
        for i in range(nc):
            o = int(words[i, 11])
            circuits.append(pkg.CircuitCheck(i, words[i], cnt[o:o + roots[i]].copy(), first[o:o + roots[i]].copy(),
                                             names[i] if names else None, origins[i] if origins else None, ext_d=4))
        return pkg.CheckReport(int(verdict.value), circuits, beta, gamma, ext_d=4)

    def lookup_balance(self, entries=64, names=None):
        """msbb_witness_lookup_balance: every message of the witness grouped by its tuple, exactly (no challenges); the groups
        whose multiplicities do not cancel modulo p, with where they came from. -> the package's LookupBalanceReport (modulus
        p) with at most `entries` entries. names (optional, per circuit): labels for the text of the report."""
        pkg = _pkg()
        sysm = self.system
        nl = [sysm.circuit_info(i)["num_lookups"] for i in range(sysm.n_circuits)]
        total = sum(nl)
        summary, counts = np.zeros(4, dtype=np.uint64), np.zeros(total + 1, dtype=np.uint64)
        ent = np.zeros((max(entries, 1), pkg.LB_ENTRY_WORDS), dtype=np.uint64)
        args_cap = 64 * max(entries, 1)
        while True:
            args = np.zeros(args_cap, dtype=np.uint32)
            _check(_lib().msbb_witness_lookup_balance(self.h, summary.ctypes.data_as(u64p), ent.ctypes.data_as(u64p), C.c_size_t(entries), _p32(args),
                                                      C.c_size_t(args_cap), counts.ctypes.data_as(u64p), C.c_size_t(total + 1)))
            n = int(summary[3])
            need = int(ent[:n, 5].sum())
            if need <= args_cap:
                break
            args_cap = need  # some tuple did not fit: the lengths are known now
        none = (1 << 64) - 1
        out = []
        for e in ent[:n]:
            origin = ("claims", int(e[1]), 0) if int(e[0]) == none else (int(e[0]), int(e[1]), int(e[2]))
            a = None if int(e[6]) == none else [int(x) for x in args[int(e[6]):int(e[6]) + int(e[5])]]
            out.append(pkg.BalanceEntry(origin, int(e[3]), int(e[4]), a, p=P))
        offs = np.cumsum([0] + nl)
        slot_counts = [[int(x) for x in counts[offs[i]:offs[i + 1]]] for i in range(sysm.n_circuits)]
        return pkg.LookupBalanceReport(int(summary[0]), int(summary[1]), int(summary[2]), out, slot_counts, int(counts[total]), names, p=P)

    def derive_multiplicities(self, targets, entries=64):
        """msbb_witness_derive_multiplicities: targets = [(circuit, lookup slot)], the provider slots whose multiplicity is one
        main-trace column (System.multiplicity_slot tells); that column is overwritten, on the device, with what the demand of
        all other messages of the witness asks of each row. -> the package's MultiplicityReport (entries with modulus p) with at
        most `entries` entries for demand no target row serves."""
        pkg = _pkg()
        tg = (pkg.MultTarget * max(len(targets), 1))(*[pkg.MultTarget(int(c), int(j)) for c, j in targets])
        summary = np.zeros(pkg.DM_SUMMARY_WORDS, dtype=np.uint64)
        ent = np.zeros((max(entries, 1), pkg.LB_ENTRY_WORDS), dtype=np.uint64)
        args_cap = 64 * max(entries, 1)
        while True:  # (a second call writes the same bytes: it is only made when some tuple did not fit)
            args = np.zeros(args_cap, dtype=np.uint32)
            _check(_lib().msbb_witness_derive_multiplicities(self.h, tg, C.c_size_t(len(targets)), summary.ctypes.data_as(u64p), ent.ctypes.data_as(u64p),
                                                             C.c_size_t(entries), _p32(args), C.c_size_t(args_cap)))
            n = int(summary[5])
            need = int(ent[:n, 5].sum())
            if need <= args_cap:
                break
            args_cap = need
        none = (1 << 64) - 1
        out = []
        for e in ent[:n]:
            origin = ("claims", int(e[1]), 0) if int(e[0]) == none else (int(e[0]), int(e[1]), int(e[2]))
            a = None if int(e[6]) == none else [int(x) for x in args[int(e[6]):int(e[6]) + int(e[5])]]
            out.append(pkg.BalanceEntry(origin, int(e[3]), int(e[4]), a, p=P))
        return pkg.MultiplicityReport(*(int(x) for x in summary[:5]), out)

    def trace(self, circuit):
        """one stage-1 trace of a device-resident witness read back (msbb_witness_trace): height x main_width, uint32, canonical"""
        need = C.c_size_t()
        rc = _lib().msbb_witness_trace(self.h, C.c_size_t(circuit), None, C.c_size_t(0), C.byref(need))
        if rc != -3:
            _check(rc)
        width = self.system.circuit_info(circuit)["main_width"]
        out = np.zeros((need.value // width, width), dtype=np.uint32)
        if need.value:
            _check(_lib().msbb_witness_trace(self.h, C.c_size_t(circuit), _p32(out), C.c_size_t(out.size), C.byref(need)))
        return out

    def __init__(self, system, traces, claims_packed, host_resident=False):
        """host_resident: the witness stays in host memory (msbb_witness_create_host) and every proof uploads it - the
        reference's timed region; the arrays are kept alive (and page-locked) by this object"""
        self.system = system
        offs, data = claims_packed
        trs = [_u32(t) for t in traces]
        n = len(trs)
        ptrs = (u32p * n)(*[_p32(t) for t in trs])
        hs = np.ascontiguousarray([t.shape[0] for t in trs], dtype=np.uint64)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        data = _u32(data)
        self.h = C.c_void_p()
        if host_resident:
            pinned = C.c_int32(0)
            _check(_lib().msbb_witness_create_host(system.h, ptrs, hs.ctypes.data_as(u64p), C.c_size_t(len(offs) - 1), offs.ctypes.data_as(u64p),
                                                   _p32(data), C.byref(pinned), C.byref(self.h)))
            self.keep, self.pinned = trs, bool(pinned.value)
        else:
            _check(_lib().msbb_witness_create(system.h, ptrs, hs.ctypes.data_as(u64p), C.c_size_t(len(offs) - 1), offs.ctypes.data_as(u64p),
                                              _p32(data), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_witness_destroy(self.h)
            self.h = None


class System:
    """System<BabyBearPoseidon2Config> + ProverKey (msbb_system)."""

    def __init__(self, ctx, blob: bytes, n_circuits):
        self.ctx, self.blob, self.n_circuits = ctx, blob, n_circuits
        a = np.frombuffer(blob, dtype=np.uint8)
        self.h = C.c_void_p()
        _check(_lib().msbb_system_create(ctx.h, a.ctypes.data_as(u8p), C.c_size_t(len(blob)), C.byref(self.h)))

    @staticmethod
    def new(ctx, params, circuit_inputs, poseidon2):
        with frontend.field(frontend.BABYBEAR):
            compiled = [frontend.compile_circuit(c) for c in circuit_inputs]
            blob = frontend.system_blob(params, compiled, poseidon2)
        return System(ctx, blob, len(compiled))

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_system_destroy(self.h)
            self.h = None

    def circuit_info(self, ci):
        o = np.zeros(9, dtype=np.uint64)
        _check(_lib().msbb_system_circuit_info(self.h, C.c_size_t(ci), o.ctypes.data_as(u64p)))
        keys = ["main_width", "pre_width", "pre_height", "num_lookups", "stage2_width", "constraint_count", "max_constraint_degree",
                "quotient_degree", "args_width"]
        return dict(zip(keys, (int(x) for x in o)))

    def check_info(self, ci):
        """msbb_system_check_info: what the witness check adds to circuit_info"""
        o = np.zeros(4, dtype=np.uint64)
        _check(_lib().msbb_system_check_info(self.h, C.c_size_t(ci), o.ctypes.data_as(u64p)))
        return dict(zip(["roots", "slots", "wave_steps", "lds_lanes"], (int(x) for x in o)))

    def multiplicity_slot(self, circuit, slot):
        """msbb_system_multiplicity_slot: may lookup slot `slot` of `circuit` be a target of Witness.derive_multiplicities?
        eligibility 0 yes / 1 its multiplicity is not one main-trace column (optionally negated) / 2 that column is read by
        another lookup expression of the circuit; column: the derived column; pull: the multiplicity is the negated column"""
        o = np.zeros(3, dtype=np.uint64)
        _check(_lib().msbb_system_multiplicity_slot(self.h, C.c_size_t(circuit), C.c_size_t(slot), o.ctypes.data_as(u64p)))
        return {"eligibility": int(o[0]), "column": int(o[1]), "pull": bool(o[2])}

    def circuit_kernels(self, ci):
        """msbb_system_circuit_kernels: KERNEL_QUOTIENT when the circuit's quotient kernel was generated and compiled, else 0"""
        f = C.c_uint32()
        _check(_lib().msbb_system_circuit_kernels(self.h, C.c_size_t(ci), C.byref(f)))
        return int(f.value)

    def preprocessed_commit(self):
        out = np.zeros(8 * 256, dtype=np.uint32)
        n = C.c_size_t()
        _check(_lib().msbb_system_preprocessed_commit(self.h, _p32(out), C.c_size_t(out.size), C.byref(n)))
        return out[: 8 * n.value].copy() if n.value else None

    def witness(self, traces, claims_packed):
        return Witness(self, traces, claims_packed)

    def host_witness(self, traces, claims_packed):
        """a SystemWitness that stays in host memory: every prove_multiple_claims uploads it (msbb_witness_create_host)"""
        return Witness(self, traces, claims_packed, host_resident=True)

    def witness_from_device(self, traces, claims_packed, stream=None):
        """A witness from traces that already lie in DEVICE memory (msbb_witness_create_device): per circuit None (inactive) or a
        2-D torch tensor on the context's device / any object with __cuda_array_interface__, of 1-, 2- or 4-byte elements read
        as unsigned canonical values, in any strided layout. Claims: the usual (offsets, data) pair in host memory. stream as
        for the Goldilocks System.witness_from_device. The inputs may be overwritten or freed as soon as the call returns."""
        pkg = _pkg()
        arr, _heights, seen = pkg._device_traces(traces, self.n_circuits, lambda i: self.circuit_info(i)["main_width"])
        offs, data = claims_packed
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        data = _u32(data)
        w = Witness.__new__(Witness)
        w.system, w.h = self, C.c_void_p()
        _check(_lib().msbb_witness_create_device(self.h, arr, C.c_size_t(len(offs) - 1), offs.ctypes.data_as(u64p), _p32(data),
                                                 pkg._producer_stream(stream, seen), C.byref(w.h)))
        return w

    def verify_multiple_claims(self, claims_packed, proof: bytes):
        """0 = accepted, otherwise the reference's VerificationError variant (MS_VERDICT_*)"""
        offs, data = claims_packed
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=np.uint32)
        a = np.frombuffer(proof, dtype=np.uint8) if proof else np.zeros(1, dtype=np.uint8)
        verdict = C.c_int32()
        _check(_lib().msbb_verify(self.h, C.c_size_t(len(offs) - 1), offs.ctypes.data_as(u64p), _p32(data), a.ctypes.data_as(u8p),
                                  C.c_size_t(len(proof)), C.byref(verdict)))
        return verdict.value

    verify = verify_multiple_claims

    def verify_batch(self, items):
        """msbb_verify_batch: `items` is a list of (claims_packed, proof), proofs as in verify_multiple_claims. -> the list of
        verdicts verify_multiple_claims gives one by one; the per-query arithmetic and the Merkle paths of the whole batch run
        on the device."""
        n = len(items)
        if n == 0:
            _check(_lib().msbb_verify_batch(self.h, C.c_size_t(0), None, None, None, None, None, None))
            return []
        keep, lens, ncl = [], np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        offp, datp, prp = (u64p * n)(), (u32p * n)(), (u8p * n)()
        for i, (claims_packed, proof) in enumerate(items):
            data = proof.to_bytes() if isinstance(proof, Proof) else bytes(proof)
            buf = np.frombuffer(data + b"\0", dtype=np.uint8)  # (a zero-length proof still needs an address)
            offs, cd = claims_packed
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
            cd = np.ascontiguousarray(cd, dtype=np.uint32) if len(cd) else np.zeros(1, dtype=np.uint32)
            keep.append((buf, offs, cd))
            lens[i], ncl[i] = len(data), len(offs) - 1
            offp[i], datp[i], prp[i] = offs.ctypes.data_as(u64p), _p32(cd), buf.ctypes.data_as(u8p)
        verdicts = np.full(n, -1, dtype=np.int32)
        _check(_lib().msbb_verify_batch(self.h, C.c_size_t(n), ncl.ctypes.data_as(u64p), offp, datp, prp, lens.ctypes.data_as(u64p),
                                        verdicts.ctypes.data_as(C.POINTER(C.c_int32))))
        return [int(v) for v in verdicts]

    def prove_multiple_claims(self, witness, want_times=False):
        times = np.zeros(6, dtype=np.float64)
        while True:
            # one output buffer per system, reused: a fresh multi-megabyte array per proof costs an mmap and its page faults
            cap = getattr(self, "_proof_cap", 1 << 22)
            out = getattr(self, "_proof_buf", None)
            if out is None or out.size != cap:
                out = self._proof_buf = np.zeros(cap, dtype=np.uint8)
            n = C.c_size_t()
            rc = _lib().msbb_prove(self.h, witness.h, out.ctypes.data_as(u8p), C.c_size_t(cap), C.byref(n),
                                   times.ctypes.data_as(C.POINTER(C.c_double)) if want_times else None)
            if rc == -3:
                self._proof_cap = n.value
                continue
            _check(rc)
            keys = ["stage1_commit", "lookup_construction", "stage2_commit", "quotient", "fri_open", "total"]
            return Proof(out[: n.value].tobytes(), dict(zip(keys, times.tolist())) if want_times else None)


# ---- Level 2: the prover's steps on device handles (include/mstark_bb.h; tests/test_gpu_bb_level2.py drives the reference's loop)
def _e4(x):
    a = _u32(x).reshape(-1)
    assert a.size == 4
    return a


class Challenger:
    """config.initialise_challenger() of the system's configuration (msbb_challenger_*): values in and out are canonical"""

    def __init__(self, system):
        self.system = system
        self.h = C.c_void_p()
        _check(_lib().msbb_challenger_create(system.h, C.byref(self.h)))

    def observe(self, elems):
        a = _u32(np.array([int(x) % P for x in elems], dtype=np.uint64))   # (Val::from_usize for the integers of the shape)
        _check(_lib().msbb_challenger_observe(self.h, _p32(a), C.c_size_t(a.size)))

    def observe_digests(self, words):
        a = _u32(words).reshape(-1)
        assert a.size % 8 == 0
        _check(_lib().msbb_challenger_observe_digests(self.h, _p32(a), C.c_size_t(a.size // 8)))

    def observe_claims(self, witness):
        _check(_lib().msbb_challenger_observe_claims(self.h, witness.h))

    def sample_ext(self):
        o = np.zeros(4, dtype=np.uint32)
        _check(_lib().msbb_challenger_sample_ext(self.h, _p32(o)))
        return tuple(int(x) for x in o)

    def sample_bits(self, bits):
        o = C.c_uint64()
        _check(_lib().msbb_challenger_sample_bits(self.h, C.c_uint32(bits), C.byref(o)))
        return o.value

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_challenger_destroy(self.h)
            self.h = None


class Trace:
    """a matrix that stays in HBM between two steps (msbb_trace)"""

    def __init__(self, h):
        self.h = h

    def info(self):
        o = np.zeros(3, dtype=np.uint64)
        _check(_lib().msbb_trace_info(self.h, o.ctypes.data_as(u64p)))
        return tuple(int(x) for x in o)

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_trace_destroy(self.h)
            self.h = None


class Committed:
    """prover data of one commitment (msbb_mmcs) with its cap"""

    def __init__(self, h, cap, shapes=None):
        self.h, self.cap, self.shapes = h, cap, shapes

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_mmcs_destroy(self.h)
            self.h = None


def _cap_buf(cap_height):
    return np.zeros(8 << cap_height, dtype=np.uint32)


def _trim_cap(cap, cap_height, max_height):
    return cap[: 8 * min(1 << cap_height, max_height)].copy()


def commit_stage1(witness, params, lde_heights):
    cap = _cap_buf(params.cap_height)
    h = C.c_void_p()
    _check(_lib().msbb_witness_commit_stage1(witness.h, _p32(cap), C.byref(h)))
    return Committed(h, _trim_cap(cap, params.cap_height, max(lde_heights)))


def claims_accumulator(witness, beta, gamma):
    o = np.zeros(4, dtype=np.uint32)
    _check(_lib().msbb_witness_claims_accumulator(witness.h, _p32(_e4(beta)), _p32(_e4(gamma)), _p32(o)))
    return tuple(int(x) for x in o)


def stage2_build(witness, n_active, beta, gamma, acc_in):
    accs = np.zeros(4 * n_active, dtype=np.uint32)
    hs = (C.c_void_p * n_active)()
    _check(_lib().msbb_stage2_build(witness.h, _p32(_e4(beta)), _p32(_e4(gamma)), _p32(_e4(acc_in)), _p32(accs), hs))
    return [tuple(int(x) for x in accs[4 * i: 4 * i + 4]) for i in range(n_active)], [Trace(C.c_void_p(h)) for h in hs]


def _commit(fn, system, params, traces, lde_heights):
    n = len(traces)
    hs = (C.c_void_p * n)(*[t.h for t in traces])
    cap = _cap_buf(params.cap_height)
    h = C.c_void_p()
    _check(fn(system.h, C.c_size_t(n), hs, _p32(cap), C.byref(h)))
    return Committed(h, _trim_cap(cap, params.cap_height, max(lde_heights)))


def pcs_commit_traces(system, params, traces):
    heights = [t.info()[0] << params.log_blowup for t in traces]
    return _commit(_lib().msbb_pcs_commit_traces, system, params, traces, heights)


def pcs_commit_ldes(system, params, ldes):
    heights = [t.info()[0] for t in ldes]
    return _commit(_lib().msbb_pcs_commit_ldes, system, params, ldes, heights)


def quotient(system, circuit, log_n, s1, s1_idx, s2, s2_idx, publics16, alpha):
    pub = _u32(publics16).reshape(-1)
    assert pub.size == 16
    h = C.c_void_p()
    _check(_lib().msbb_quotient(system.h, C.c_size_t(circuit), C.c_uint32(log_n), s1.h, C.c_size_t(s1_idx), s2.h, C.c_size_t(s2_idx), _p32(pub),
                                _p32(_e4(alpha)), C.byref(h)))
    return Trace(h)


def preprocessed_mmcs(system):
    h = C.c_void_p()
    _check(_lib().msbb_system_preprocessed_mmcs(system.h, C.byref(h)))
    return Committed(h, system.preprocessed_commit()) if h.value else None


def pcs_open(system, rounds, challenger):
    """rounds: [(Committed, [widths], [[point, ...] per matrix])]; returns (opened canonical words, FriProof bytes)"""
    hs = (C.c_void_p * len(rounds))(*[r[0].h for r in rounds])
    npts, pts, words = [], [], 0
    for _, widths, points in rounds:
        assert len(widths) == len(points)
        for w, ps in zip(widths, points):
            npts.append(len(ps))
            for p_ in ps:
                pts.extend(int(x) for x in p_)
            words += 4 * w * len(ps)
    npts = np.ascontiguousarray(npts, dtype=np.uint64)
    pts = _u32(pts if pts else [0])
    opened = np.zeros(max(words, 1), dtype=np.uint32)
    cap = 1 << 20
    while True:
        fri = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t()
        rc = _lib().msbb_pcs_open(system.h, C.c_size_t(len(rounds)), hs, npts.ctypes.data_as(u64p), _p32(pts), challenger.h, _p32(opened),
                                  C.c_size_t(opened.size), fri.ctypes.data_as(u8p), C.c_size_t(cap), C.byref(n))
        if rc == -3 and n.value > cap:
            raise _pkg().MstarkError("msbb_pcs_open: FriProof larger than the buffer (%d bytes); the challenger has been advanced" % n.value)
        _check(rc)
        return opened[:words].copy(), fri[: n.value].tobytes()


# ---- PCS-level entry points
def set_poseidon2(ctx, constants141):
    k = _u32(constants141).reshape(-1)
    assert k.size == 141
    _check(_lib().msbb_set_poseidon2(ctx.h, _p32(k)))


def poseidon2_permute(ctx, states):
    st = _u32(states).reshape(-1, 16).copy()
    _check(_lib().msbb_poseidon2_permute(ctx.h, _p32(st), C.c_size_t(st.shape[0])))
    return st


def dft_batch(ctx, m, inverse=False):
    m = _u32(m)
    out = np.empty_like(m)
    _check(_lib().msbb_dft_batch(ctx.h, _p32(m), C.c_size_t(m.shape[0]), C.c_size_t(m.shape[1]), C.c_int32(int(inverse)), _p32(out)))
    return out


def coset_lde_batch(ctx, m, log_blowup):
    m = _u32(m)
    out = np.empty((m.shape[0] << log_blowup, m.shape[1]), dtype=np.uint32)
    _check(_lib().msbb_coset_lde_batch(ctx.h, _p32(m), C.c_size_t(m.shape[0]), C.c_size_t(m.shape[1]), C.c_uint32(log_blowup), _p32(out)))
    return out


class Mmcs:
    def __init__(self, ctx, mats, cap_height=0):
        self.ctx = ctx
        self.mats = [_u32(m) for m in mats]
        n = len(self.mats)
        ptrs = (u32p * n)(*[_p32(m) for m in self.mats])
        hs = np.ascontiguousarray([m.shape[0] for m in self.mats], dtype=np.uint64)
        ws = np.ascontiguousarray([m.shape[1] for m in self.mats], dtype=np.uint64)
        maxh = int(hs.max())
        cap = np.zeros(8 << cap_height, dtype=np.uint32)
        self.h = C.c_void_p()
        _check(_lib().msbb_mmcs_commit(ctx.h, C.c_size_t(n), ptrs, hs.ctypes.data_as(u64p), ws.ctypes.data_as(u64p), C.c_uint32(cap_height),
                                       _p32(cap), C.byref(self.h)))
        self.cap = cap[: 8 * min(1 << cap_height, maxh)].copy()
        self.widths, self.log_max = ws, maxh.bit_length() - 1

    def open(self, index):
        vals = np.zeros(int(self.widths.sum()), dtype=np.uint32)
        proof = np.zeros(8 * (self.log_max + 1), dtype=np.uint32)
        k = C.c_size_t()
        _check(_lib().msbb_mmcs_open(self.h, C.c_size_t(index), _p32(vals), _p32(proof), C.byref(k)))
        return vals, proof[: 8 * k.value].copy()

    def verify_batch(self, indices, vals, siblings):
        """MerkleTreeMmcs::verify_batch of many openings of this commitment on the device (msbb_mmcs_verify_batch): per
        opening its index, the values and the sibling words `open` returns. -> np.ndarray of 0 / 1"""
        hs = [m.shape[0] for m in self.mats]
        return mmcs_verify_batch(self.ctx, self.cap, self.cap.size // 8, hs, self.widths, indices, vals, siblings)

    def __del__(self):
        if getattr(self, "h", None):
            _lib().msbb_mmcs_destroy(self.h)
            self.h = None


def _raw32(a):
    """u32 words as they are: a word >= p is the entry point's to refuse, not an error of the call"""
    return np.ascontiguousarray(np.asarray(a).ravel(), dtype=np.uint32)


def mmcs_verify_batch(ctx, cap, cap_size, heights, widths, indices, vals, siblings):
    """msbb_mmcs_verify_batch without an Mmcs: the commitment is its cap (`cap_size` digests of 8 words), heights and widths.
    indices: n integers; vals: per opening the rows concatenated in matrix order; siblings: per opening its path words."""
    hs = np.ascontiguousarray(heights, dtype=np.uint64)
    ws = np.ascontiguousarray(widths, dtype=np.uint64)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    n = idx.size
    rw = int(ws.sum())
    cap = _raw32(cap)
    cap_height = int(cap_size).bit_length() - 1
    if cap_size != 1 << cap_height or cap.size != 8 * cap_size:
        raise _pkg().MstarkError("a cap holds a power-of-two number of 8-word digests")
    path = max(int(hs.max()).bit_length() - 1 - cap_height, 0) if hs.size else 0
    v = np.zeros(max(n * rw, 1), dtype=np.uint32)
    if n * rw:
        v[: n * rw] = np.concatenate([_raw32(x) for x in vals]) if not isinstance(vals, np.ndarray) else _raw32(vals)
    sib = np.zeros(max(n * path * 8, 1), dtype=np.uint32)
    flat = (np.concatenate([_raw32(s) for s in siblings]) if not isinstance(siblings, np.ndarray) else _raw32(siblings)) if n else np.zeros(0, dtype=np.uint32)
    if flat.size != n * path * 8:
        raise _pkg().MstarkError("expected %d sibling words per opening" % (path * 8))
    sib[: flat.size] = flat
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _check(_lib().msbb_mmcs_verify_batch(ctx.h, C.c_size_t(hs.size), hs.ctypes.data_as(u64p), ws.ctypes.data_as(u64p), _p32(cap),
                                         C.c_uint32(cap_height), C.c_size_t(n),
                                         (idx if n else np.zeros(1, dtype=np.uint64)).ctypes.data_as(u64p), _p32(v), _p32(sib),
                                         ok.ctypes.data_as(u8p)))
    return ok[:n].copy()


def field_op(ctx, op, a, b=None):
    a = _u32(a)
    out = np.empty_like(a)
    n = a.size // 4 if op >= 4 else a.size
    bb = _u32(b) if b is not None else None
    _check(_lib().msbb_field_op(ctx.h, C.c_int32(op), _p32(a), _p32(bb) if bb is not None else None, C.c_size_t(n), _p32(out)))
    return out
