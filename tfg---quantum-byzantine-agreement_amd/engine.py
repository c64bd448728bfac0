"""Device engine: torch-tensor front end of libqba (include/qba.h).

PyTorch is used only for device memory, streams and torch.distributed; every
computation on lists, counts and statevectors runs in the HIP kernels of
libqba.  Constructing an :class:`Engine` without the library or without a
gfx950 GPU raises :class:`QbaError` -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import resource
from ._lib import KIND_NOTQ, KIND_Q, MAX_PARTIES, GridScenario, QbaError, Scenario, call, lib


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _u64(x) -> int:
    """A seed or an instance index as the uint64 the library takes (mod 2^64)."""
    return int(x) & ((1 << 64) - 1)


def _row_ld(nbytes: int) -> int:
    """Row pitch of a list buffer whose rows hold ``nbytes`` bytes."""
    # rows start 4 KiB-aligned: the 8-B-per-lane row stores then never
    # straddle a partial line at a row start (1.3% over 64-B alignment at
    # n = 11, measured in round 2)
    return max(4096, (nbytes + 4095) // 4096 * 4096)


def _packet_stage(stage: np.ndarray, off: int, order, rows) -> int:
    """Writes the stage of one packet request, [order | rows] (every row
    len(order) entries), into ``stage`` at ``off``; returns the offset behind it."""
    ln = len(order)
    stage[off:off + ln] = order
    for t in rows:
        off += ln
        stage[off:off + ln] = t if isinstance(t, np.ndarray) else np.fromiter(t, dtype=np.int64, count=ln)
    return off + ln


def _packet_result(out: np.ndarray, o: int, ln: int, m: int, who: str) -> Tuple[np.ndarray, bool]:
    """(own as the int64 array it travels as, verdict) from one packet's
    output at out[o:]: own (ln), bad index, violation among the rows,
    violation of own, eq (m), as qba_check_packet writes them."""
    e = o + ln
    if out[e]:
        raise QbaError(f"{who}: index outside the list")
    eq = out[e + 3:e + 3 + m]
    ok = not out[e + 1] and not out[e + 2] and bool(np.all((eq == 0) | (eq == ln)))
    if m and not ln:  # every tuple empty: the set is {()}, vacuously consistent
        ok = True
    return out[o:e], ok


@dataclass
class Counts:
    """Count-mode result of one pass (see qba.h): int64 device tensors."""

    H: torch.Tensor  # [w][n+1][w]
    C: torch.Tensor  # [w][n+1][n+1]
    P: torch.Tensor  # [w]

    def numpy(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self.H.cpu().numpy(), self.C.cpu().numpy(), self.P.cpu().numpy()


class Engine:
    """One libqba context bound to one GPU."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise QbaError("no GPU visible: the qba engine has no CPU fallback")
        self.device = torch.device("cuda", device)
        self.index = device
        handle = C.c_void_p()
        torch.cuda.set_device(device)
        call("qba_init", device, C.byref(handle))
        self._ctx = handle
        self._prepared: Dict[int, dict] = {}

    # -- lifetime ----------------------------------------------------------
    def close(self) -> None:
        if self._ctx:
            torch.cuda.synchronize(self.device)
            call("qba_destroy", self._ctx)
            self._ctx = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            if getattr(self, "_ctx", None):
                lib().qba_destroy(self._ctx)
        except Exception:
            pass

    @property
    def ctx(self) -> C.c_void_p:
        if not self._ctx:
            raise QbaError("engine closed")
        return self._ctx

    def stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- sizes --------------------------------------------------------------
    @staticmethod
    def sizes(n: int) -> Tuple[int, int]:
        nq = resource.n_qubits(n)
        return nq, 1 << nq

    @staticmethod
    def _check_n(n: int) -> None:
        if not 1 <= n <= MAX_PARTIES:
            raise QbaError(f"n_parties={n} outside [1, {MAX_PARTIES}]")

    # -- (A1/A2) resource preparation ------------------------------------------
    def prepare(self, n: int, perm: Optional[Sequence[int]] = None) -> dict:
        """Compile both reference circuits for n parties (tfg.py:15-65).

        The Q circuit is built with permutation ``perm`` (default: identity);
        its X gates are verified by the library to be the classical mask the
        sampler redraws for every entry.
        """
        self._check_n(n)
        if n in self._prepared and perm is None:
            return self._prepared[n]
        nq, _ = self.sizes(n)
        notq = resource.notQCorrelated(n, nq)
        q = resource.qCorrelated(n, nq, perm=list(range(1, n + 1)) if perm is None else perm)
        return self.compile(n, notq, q)

    def compile(self, n: int, notq: "resource.Gate", q: "resource.Gate") -> dict:
        """Compile a (not-Q, Q) circuit pair for n parties and make it the
        program that sample / sample_check use for n.  ``q.perm`` is the
        permutation its X gates encode.  Returns the program info (tables and
        the sampler flags: canonical table layout, closed form)."""
        self._check_n(n)
        nq, _ = self.sizes(n)
        g0 = np.ascontiguousarray(notq.triples())
        g1 = np.ascontiguousarray(q.triples())
        p1 = np.ascontiguousarray(np.asarray(q.perm, dtype=np.int32))
        call("qba_resource_compile", self.ctx, n, KIND_NOTQ, _i32p(g0), len(g0), None)
        call("qba_resource_compile", self.ctx, n, KIND_Q, _i32p(g1), len(g1), _i32p(p1))
        flags = np.zeros(6, np.int32)
        call("qba_program_flags", self.ctx, n, _i32p(flags))
        info = {"n": n, "nq": nq, "notq": self.program(n, KIND_NOTQ), "q": self.program(n, KIND_Q),
                "canonical": bool(flags[0]), "closed": bool(flags[1])}
        self._prepared[n] = info
        return info

    def program(self, n: int, kind: int) -> dict:
        nf = C.c_int32()
        tl = C.c_int32()
        desc = np.zeros((16, 6), np.int32)
        cap = 8192
        pat = np.zeros(cap, np.uint64)
        apat = np.zeros(cap, np.uint64)
        thr = np.zeros(cap, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        call("qba_program_export", self.ctx, n, kind, C.byref(nf), _i32p(desc),
             pat.ctypes.data_as(u64p), apat.ctypes.data_as(u64p), thr.ctypes.data_as(u64p), cap,
             C.byref(tl))
        t = tl.value
        return {"nfac": nf.value, "desc": desc[: nf.value].copy(), "pat": pat[:t].copy(),
                "apat": apat[:t].copy(), "thr": thr[:t].copy()}

    # -- buffers -----------------------------------------------------------------
    def alloc_lists(self, n: int, count: int) -> torch.Tensor:
        return torch.empty((n + 1, _row_ld(count)), dtype=torch.uint8, device=self.device)

    def alloc_packed(self, n: int, count: int) -> torch.Tensor:
        """Nibble rows (qba.h "packed lists"): (count + 1) // 2 bytes per row,
        rows 4 KiB-aligned like alloc_lists."""
        return torch.empty((n + 1, _row_ld((count + 1) // 2)), dtype=torch.uint8, device=self.device)

    def alloc_counts(self, n: int) -> Counts:
        _, w = self.sizes(n)
        z = lambda *s: torch.zeros(s, dtype=torch.int64, device=self.device)  # noqa: E731
        return Counts(z(w, n + 1, w), z(w, n + 1, n + 1), z(w))

    @staticmethod
    def _lists_ok(lists: torch.Tensor, n: int, count: int) -> int:
        if lists.dtype != torch.uint8 or lists.dim() != 2 or lists.shape[0] != n + 1:
            raise QbaError("lists must be a uint8 [n+1, ld] device tensor")
        if lists.stride(1) != 1 or lists.shape[1] < count:
            raise QbaError("lists rows must be contiguous and hold `count` entries")
        return lists.stride(0)

    @staticmethod
    def _packed_ok(packed: torch.Tensor, rows: int, count: int) -> int:
        if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[0] != rows:
            raise QbaError(f"packed lists must be a uint8 [{rows}, ld] device tensor")
        if packed.stride(1) != 1 or packed.shape[1] < (count + 1) // 2:
            raise QbaError("packed rows must be contiguous and hold (count + 1) // 2 bytes")
        return packed.stride(0)

    # -- (A3/A4) sampling ---------------------------------------------------------
    def sample(self, n: int, seed: int, first: int, count: int,
               lists: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Lists of entries [first, first+count) (tfg.py:68-84, 128-129)."""
        self.prepare(n)
        if lists is None:
            lists = self.alloc_lists(n, count)
        ld = self._lists_ok(lists, n, count)
        call("qba_sample", self.ctx, n, seed, first, count, _ptr(lists), ld, self.stream())
        return lists

    def sample_check(self, n: int, seed: int, first: int, count: int,
                     lists: Optional[torch.Tensor] = None, counts: Optional[Counts] = None,
                     accumulate: bool = False, deferred: bool = False) -> Tuple[torch.Tensor, Counts]:
        """deferred: qba_sample_check_deferred -- the counts are complete only
        after the next deferred call or flush_deferred() (include/qba.h)."""
        self.prepare(n)
        if lists is None:
            lists = self.alloc_lists(n, count)
        if counts is None:
            counts = self.alloc_counts(n)
        ld = self._lists_ok(lists, n, count)
        call("qba_sample_check_deferred" if deferred else "qba_sample_check", self.ctx, n, seed, first, count,
             _ptr(lists), ld, _ptr(counts.H), _ptr(counts.C), _ptr(counts.P), int(accumulate), self.stream())
        return lists, counts

    def flush_deferred(self) -> None:
        """Launch the pending deferred reduction (on its call's stream)."""
        call("qba_flush_deferred", self.ctx)

    def sample_packed(self, n: int, seed: int, first: int, count: int,
                      packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sample() into nibble rows."""
        self.prepare(n)
        if packed is None:
            packed = self.alloc_packed(n, count)
        ld = self._packed_ok(packed, n + 1, count)
        call("qba_sample_packed", self.ctx, n, seed, first, count, _ptr(packed), ld, self.stream())
        return packed

    def sample_check_packed(self, n: int, seed: int, first: int, count: int,
                            packed: Optional[torch.Tensor] = None, counts: Optional[Counts] = None,
                            accumulate: bool = False, deferred: bool = False) -> Tuple[torch.Tensor, Counts]:
        """The fused hot path writing nibble rows (half the bytes of
        sample_check; same lists and counts).  deferred: as sample_check."""
        self.prepare(n)
        if packed is None:
            packed = self.alloc_packed(n, count)
        if counts is None:
            counts = self.alloc_counts(n)
        ld = self._packed_ok(packed, n + 1, count)
        call("qba_sample_check_packed_deferred" if deferred else "qba_sample_check_packed", self.ctx, n, seed,
             first, count, _ptr(packed), ld, _ptr(counts.H), _ptr(counts.C), _ptr(counts.P), int(accumulate),
             self.stream())
        return packed, counts

    def sample_check_batched(self, n: int, seed_base: int, n_inst: int, count: int,
                             lists: Optional[torch.Tensor] = None,
                             packed: bool = False, flip_q16: int = 0) -> Tuple[torch.Tensor, Counts]:
        """n_inst independent runs (key seed_base + i) of `count` entries each.
        Returns lists [n_inst, n+1, ld] (nibble rows when packed) and
        per-instance counts [n_inst, ...].  ``flip_q16=k > 0``
        (qba_sample_check_batched_noisy / _packed_noisy): every measured bit of
        an entry flips with probability k / 65536 (montecarlo.noise_masks) as
        it is sampled; the lists and the counts are those of the noisy entries."""
        flip = self._check_flip(flip_q16)
        self.prepare(n)
        _, w = self.sizes(n)
        nb = (count + 1) // 2 if packed else count
        if lists is None:
            lists = torch.empty((n_inst, n + 1, _row_ld(nb)), dtype=torch.uint8, device=self.device)
        if lists.dim() != 3 or lists.shape[:2] != (n_inst, n + 1) or lists.stride(2) != 1:
            raise QbaError("lists must be a uint8 [n_inst, n+1, ld] tensor")
        z = lambda *s: torch.empty(s, dtype=torch.int64, device=self.device)  # noqa: E731
        counts = Counts(z(n_inst, w, n + 1, w), z(n_inst, w, n + 1, n + 1), z(n_inst, w))
        if lists.shape[2] < nb:
            raise QbaError("lists rows too short for `count` entries")
        name = "qba_sample_check_batched_packed" if packed else "qba_sample_check_batched"
        rest = (_ptr(lists), lists.stride(1), lists.stride(0), _ptr(counts.H), _ptr(counts.C), _ptr(counts.P),
                self.stream())
        if flip:
            call(name + "_noisy", self.ctx, n, _u64(seed_base), n_inst, count, flip, *rest)
        else:  # (ctypes reduces the seed mod 2^64 as _u64 does)
            call(name, self.ctx, n, _u64(seed_base), n_inst, count, *rest)
        return lists, counts

    @staticmethod
    def _check_adversary(adversary) -> Optional[int]:
        """None, or the checked policy word (montecarlo.adversary; DESIGN.md
        section 13.7) that sends a call to its ``_adv`` entry point."""
        if adversary is None:
            return None
        from .montecarlo import check_adversary
        return check_adversary(adversary)

    def protocol_batched(self, n: int, n_dishonest: int, seed_base: int, counts: Counts,
                         out: Optional[torch.Tensor] = None, adversary: Optional[int] = None) -> torch.Tensor:
        """The protocol rounds of every instance of ``counts`` (the per-instance
        tables of sample_check_batched) in one launch (tfg.py:101-125, 166-196,
        266-306, 337-363): int32 [n_inst, 4 + 5*(n+1)], layout in qba.h.
        ``adversary=word`` (qba_protocol_batched_adv): the dishonest parties
        follow that policy (montecarlo.adversary); None is the reference's rule
        through the call that existed before, 0xF the same rows."""
        self._check_n(n)
        adv = self._check_adversary(adversary)
        _, w = self.sizes(n)
        g = n + 1
        n_inst = counts.P.shape[0] if counts.P.dim() == 2 else -1
        for t, shape in ((counts.H, (n_inst, w, g, w)), (counts.C, (n_inst, w, g, g)), (counts.P, (n_inst, w))):
            if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                    t.device != self.device:
                raise QbaError("counts must be contiguous int64 [n_inst, ...] tensors of sample_check_batched")
        out = self._rows_out(n, n_inst, out)
        if adv is not None:
            call("qba_protocol_batched_adv", self.ctx, n, n_dishonest, seed_base, n_inst, _ptr(counts.H),
                 _ptr(counts.C), _ptr(counts.P), _ptr(out), self.stream(), adv)
            return out
        call("qba_protocol_batched", self.ctx, n, n_dishonest, seed_base, n_inst, _ptr(counts.H), _ptr(counts.C),
             _ptr(counts.P), _ptr(out), self.stream())
        return out

    def _rows_out(self, n: int, n_inst: int, out: Optional[torch.Tensor], k: Optional[int] = None) -> torch.Tensor:
        """``out``, or a new buffer when it is None: result rows [n_inst, words],
        or [k, n_inst, words] of a curve call."""
        shape = (n_inst, 4 + 5 * (n + 1)) if k is None else (k, n_inst, 4 + 5 * (n + 1))
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != shape or \
                not out.is_contiguous() or out.device != self.device:
            raise QbaError(f"out must be a contiguous int32 {list(shape)} device tensor")
        return out

    CURVE_MAX = 32  # QBA_MC_CURVE_MAX

    @classmethod
    def _check_curve(cls, n: int, n_dishonest: int, n_inst: int, counts) -> list:
        """The argument check of the four montecarlo_* methods; returns the
        checkpoints as a list of ints.  A single-count call is ``[count]``."""
        try:
            cs = [int(c) for c in counts]
        except TypeError:
            raise QbaError("counts must be a sequence of integers") from None
        if not 0 <= n_dishonest <= n:
            raise QbaError(f"n_dishonest={n_dishonest} outside [0, {n}]")
        if not 1 <= len(cs) <= cls.CURVE_MAX:
            raise QbaError(f"between 1 and {cls.CURVE_MAX} checkpoints, not {len(cs)}")
        if any(b <= a for a, b in zip(cs, cs[1:])) or cs[0] < 0 or cs[-1] >= 1 << 31:
            raise QbaError("counts must be strictly increasing, with 0 <= counts[0] and counts[-1] < 2^31")
        if n_inst < 0:
            raise QbaError("n_inst >= 0")
        return cs

    def _mc_lists(self, n: int, lists, need: int):
        """Injected lists, a uint8 [n_inst, n+1, >= need] device tensor or a
        host array of that shape (copied to the device), as ``(lists, n_inst,
        ld, inst_stride)``."""
        if isinstance(lists, np.ndarray):
            lists = torch.from_numpy(np.array(lists, dtype=np.uint8, order="C")).to(self.device)  # a writable copy
        if not isinstance(lists, torch.Tensor) or lists.dtype != torch.uint8 or lists.dim() != 3 or \
                lists.shape[1] != n + 1 or lists.device != self.device or \
                (lists.numel() and lists.stride(2) != 1) or lists.shape[2] < need:
            raise QbaError(f"lists must be a uint8 [n_inst, n+1, >= {need}] device tensor with unit column stride")
        n_inst = lists.shape[0]
        ld, stride = (lists.stride(1), lists.stride(0)) if lists.numel() else (need, (n + 1) * need)
        if need and n_inst and (ld < need or (n_inst > 1 and stride < (n + 1) * ld)):
            raise QbaError(f"lists rows overlap: need stride(1) >= {need} and stride(0) >= (n+1)*stride(1)")
        return lists, n_inst, ld, stride

    @staticmethod
    def _check_flip(flip_q16: int) -> int:
        if not 0 <= int(flip_q16) <= 65535:
            raise QbaError("flip_q16 must be in [0, 65535]")
        return int(flip_q16)

    def montecarlo_sampled(self, n: int, n_dishonest: int, seed_base: int, n_inst: int, count: int,
                           out: Optional[torch.Tensor] = None, flip_q16: int = 0,
                           adversary: Optional[int] = None) -> torch.Tensor:
        """n_inst instances (key seed_base + i) of `count` entries sampled,
        distilled and decided in one kernel (qba_montecarlo_sampled): the rows
        of protocol_batched(sample_check_batched(...)), int32
        [n_inst, 4 + 5*(n+1)], with no list buffer and no count tables.
        ``flip_q16=k > 0`` (qba_montecarlo_sampled_noisy): every measured bit of
        an entry flips with probability k / 65536 first (montecarlo.noise_masks).
        ``adversary=word`` (qba_montecarlo_sampled_adv, with or without noise):
        as in protocol_batched."""
        self._check_n(n)
        self._check_curve(n, n_dishonest, n_inst, [count])
        flip = self._check_flip(flip_q16)
        adv = self._check_adversary(adversary)
        self.prepare(n)
        out = self._rows_out(n, n_inst, out)
        if adv is not None:
            call("qba_montecarlo_sampled_adv", self.ctx, n, n_dishonest, _u64(seed_base), n_inst, count, flip,
                 _ptr(out), self.stream(), adv)
        elif flip:
            call("qba_montecarlo_sampled_noisy", self.ctx, n, n_dishonest, _u64(seed_base), n_inst, count, flip,
                 _ptr(out), self.stream())
        else:
            call("qba_montecarlo_sampled", self.ctx, n, n_dishonest, _u64(seed_base), n_inst, count, _ptr(out),
                 self.stream())
        return out

    def noise_apply(self, n: int, seed_base: int, lists: torch.Tensor, count: int, flip_q16: int) -> torch.Tensor:
        """XOR the flips of ``flip_q16`` (montecarlo.noise_masks under key
        seed_base + i) into columns [0, count) of the uint8 [n_inst, n+1, ld]
        device lists of sample_check_batched, in place
        (qba_noise_apply_batched); returns ``lists``."""
        self._check_n(n)
        flip = self._check_flip(flip_q16)
        if not isinstance(lists, torch.Tensor) or lists.dtype != torch.uint8 or lists.dim() != 3 or \
                lists.shape[1] != n + 1 or lists.device != self.device or lists.stride(2) != 1 or \
                lists.shape[2] < count:
            raise QbaError("lists must be a uint8 [n_inst, n+1, >= count] device tensor with unit column stride")
        call("qba_noise_apply_batched", self.ctx, n, _u64(seed_base), lists.shape[0], count, flip, _ptr(lists),
             lists.stride(1), lists.stride(0), self.stream())
        return lists

    def montecarlo_lists(self, n: int, n_dishonest: int, seed_base: int, lists, count: int,
                         out: Optional[torch.Tensor] = None, adversary: Optional[int] = None) -> torch.Tensor:
        """The same rows from injected lists (qba_montecarlo_lists): a uint8
        [n_inst, n+1, >= count] device tensor in the layout of
        sample_check_batched, or a host array of that shape (copied to the
        device).  A row's status 4 marks a value >= w at a Q-correlated
        position (montecarlo.ST_RANGE).  ``adversary=word``
        (qba_montecarlo_lists_adv): as in protocol_batched."""
        self._check_n(n)
        self._check_curve(n, n_dishonest, 0, [count])
        adv = self._check_adversary(adversary)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, count)
        out = self._rows_out(n, n_inst, out)
        if adv is not None:
            call("qba_montecarlo_lists_adv", self.ctx, n, n_dishonest, _u64(seed_base), n_inst, count, _ptr(lists), ld,
                 stride, _ptr(out), self.stream(), adv)
            return out
        call("qba_montecarlo_lists", self.ctx, n, n_dishonest, _u64(seed_base), n_inst, count, _ptr(lists), ld, stride,
             _ptr(out), self.stream())
        return out

    # -- a whole sizeL curve in one pass (qba_montecarlo_curve_*) ------------------
    def montecarlo_curve_sampled(self, n: int, n_dishonest: int, seed_base: int, n_inst: int, counts,
                                 out: Optional[torch.Tensor] = None, flip_q16: int = 0,
                                 adversary: Optional[int] = None) -> torch.Tensor:
        """The n_inst instances of montecarlo_sampled decided at every count of
        the strictly increasing ``counts`` (at most 32) in one pass over their
        entries (qba_montecarlo_curve_sampled): int32 [len(counts), n_inst,
        4 + 5*(n+1)], slice j word for word montecarlo_sampled(count=counts[j]),
        with ``flip_q16`` as there (qba_montecarlo_curve_sampled_noisy) and
        ``adversary`` as there (qba_montecarlo_curve_sampled_adv)."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, n_inst, counts)
        flip = self._check_flip(flip_q16)
        adv = self._check_adversary(adversary)
        self.prepare(n)
        out = self._rows_out(n, n_inst, out, len(cs))
        if adv is not None:
            call("qba_montecarlo_curve_sampled_adv", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
                 (C.c_uint32 * len(cs))(*cs), len(cs), flip, _ptr(out), self.stream(), adv)
        elif flip:
            call("qba_montecarlo_curve_sampled_noisy", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
                 (C.c_uint32 * len(cs))(*cs), len(cs), flip, _ptr(out), self.stream())
        else:
            call("qba_montecarlo_curve_sampled", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
                 (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(out), self.stream())
        return out

    def montecarlo_curve_lists(self, n: int, n_dishonest: int, seed_base: int, lists, counts,
                               out: Optional[torch.Tensor] = None, adversary: Optional[int] = None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_curve_lists), uint8
        [n_inst, n+1, >= counts[-1]] as montecarlo_lists takes them: slice j is
        montecarlo_lists(count=counts[j]).  A value >= w at Q-correlated
        position k gives status 4 in exactly the slices with counts[j] > k.
        ``adversary=word`` (qba_montecarlo_curve_lists_adv): as in protocol_batched."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, 0, counts)
        adv = self._check_adversary(adversary)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._rows_out(n, n_inst, out, len(cs))
        if adv is not None:
            call("qba_montecarlo_curve_lists_adv", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
                 (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(lists), ld, stride, _ptr(out), self.stream(), adv)
            return out
        call("qba_montecarlo_curve_lists", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(lists), ld, stride, _ptr(out), self.stream())
        return out

    # -- the curve with colluding traitors (qba_montecarlo_curve_*_coal) -----------
    @staticmethod
    def _check_coalition(coalition) -> int:
        """A coalition word (None: 0, no coalition) checked on the host."""
        from .montecarlo import check_coalition
        return 0 if coalition is None else check_coalition(coalition)

    def montecarlo_curve_sampled_coal(self, n: int, n_dishonest: int, seed_base: int, n_inst: int, counts,
                                      out: Optional[torch.Tensor] = None, flip_q16: int = 0,
                                      adversary: Optional[int] = None, coalition: Optional[int] = None) -> torch.Tensor:
        """montecarlo_curve_sampled with colluding traitors
        (qba_montecarlo_curve_sampled_coal): the same rows layout, the
        dishonest parties under the policy ``adversary`` (None: the reference's
        0xF) and the coalition word ``coalition`` (montecarlo.coalition; None
        or 0: no coalition, the rows of the ``adversary`` call)."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, n_inst, counts)
        flip = self._check_flip(flip_q16)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        coal = self._check_coalition(coalition)
        self.prepare(n)
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_sampled_coal", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), flip, _ptr(out), self.stream(), adv, coal)
        return out

    def montecarlo_curve_lists_coal(self, n: int, n_dishonest: int, seed_base: int, lists, counts,
                                    out: Optional[torch.Tensor] = None, adversary: Optional[int] = None,
                                    coalition: Optional[int] = None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_curve_lists_coal), as
        montecarlo_curve_lists takes them."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, 0, counts)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        coal = self._check_coalition(coalition)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_lists_coal", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(lists), ld, stride, _ptr(out), self.stream(), adv, coal)
        return out

    # -- the curve on a network that loses packets (qba_montecarlo_curve_*_net) -----
    @staticmethod
    def _check_net(net) -> int:
        """A network word (None: 0, the perfect network) checked on the host."""
        from .montecarlo import check_net
        return 0 if net is None else check_net(net)

    def montecarlo_curve_sampled_net(self, n: int, n_dishonest: int, seed_base: int, n_inst: int, counts,
                                     out: Optional[torch.Tensor] = None, flip_q16: int = 0,
                                     adversary: Optional[int] = None, net: Optional[int] = None) -> torch.Tensor:
        """montecarlo_curve_sampled on lossy links
        (qba_montecarlo_curve_sampled_net): the same rows layout, the dishonest
        parties under the policy ``adversary`` (None: the reference's 0xF) and
        packets lost as the network word ``net`` says (montecarlo.net; None or
        0: the perfect network, the rows of the ``adversary`` call)."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, n_inst, counts)
        flip = self._check_flip(flip_q16)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        word = self._check_net(net)
        self.prepare(n)
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_sampled_net", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), flip, _ptr(out), self.stream(), adv, word)
        return out

    def montecarlo_curve_lists_net(self, n: int, n_dishonest: int, seed_base: int, lists, counts,
                                   out: Optional[torch.Tensor] = None, adversary: Optional[int] = None,
                                   net: Optional[int] = None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_curve_lists_net), as
        montecarlo_curve_lists takes them."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, 0, counts)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        word = self._check_net(net)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_lists_net", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(lists), ld, stride, _ptr(out), self.stream(), adv, word)
        return out

    # -- the curve under a noise profile (qba_montecarlo_curve_*_nprof) ------------
    @staticmethod
    def _check_noise(n: int, noise):
        """A noise profile ``(rates, depol_q16)`` (None: all zero) checked on the
        host, as the calls take it: ``(uint16 array, n + 1, depol_q16)``."""
        from .montecarlo import check_noise_profile
        rates, depol = check_noise_profile(n, *(((0,) * (n + 1), 0) if noise is None else noise))
        return (C.c_uint16 * len(rates))(*rates), len(rates), depol

    def montecarlo_curve_sampled_nprof(self, n: int, n_dishonest: int, seed_base: int, n_inst: int, counts,
                                       out: Optional[torch.Tensor] = None, adversary: Optional[int] = None,
                                       noise=None) -> torch.Tensor:
        """montecarlo_curve_sampled under a noise profile
        (qba_montecarlo_curve_sampled_nprof): the same rows layout, the
        dishonest parties under the policy ``adversary`` (None: the reference's
        0xF) and every entry XORed with the masks of ``noise`` = ``(rates,
        depol_q16)`` (montecarlo.noise_masks_profile; None: the all-zero
        profile, the rows of the ``adversary`` call without noise)."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, n_inst, counts)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        rates, n_rates, depol = self._check_noise(n, noise)
        self.prepare(n)
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_sampled_nprof", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(out), self.stream(), adv, rates, n_rates, depol)
        return out

    def montecarlo_curve_lists_nprof(self, n: int, n_dishonest: int, seed_base: int, lists, counts,
                                     out: Optional[torch.Tensor] = None, adversary: Optional[int] = None,
                                     noise=None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_curve_lists_nprof), as
        montecarlo_curve_lists takes them: the masks are XORed into the rows as
        the kernel reads them, ``lists`` stays as it is."""
        self._check_n(n)
        cs = self._check_curve(n, n_dishonest, 0, counts)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        rates, n_rates, depol = self._check_noise(n, noise)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._rows_out(n, n_inst, out, len(cs))
        call("qba_montecarlo_curve_lists_nprof", self.ctx, n, n_dishonest, _u64(seed_base), n_inst,
             (C.c_uint32 * len(cs))(*cs), len(cs), _ptr(lists), ld, stride, _ptr(out), self.stream(), adv, rates,
             n_rates, depol)
        return out

    def noise_profile_apply(self, n: int, seed_base: int, lists: torch.Tensor, count: int, noise) -> torch.Tensor:
        """XOR the masks of the profile ``noise`` = ``(rates, depol_q16)``
        (montecarlo.noise_masks_profile under key seed_base + i) into columns
        [0, count) of the uint8 [n_inst, n+1, ld] device lists of
        sample_check_batched, in place (qba_noise_profile_apply); returns
        ``lists``."""
        self._check_n(n)
        rates, n_rates, depol = self._check_noise(n, noise)
        if not isinstance(lists, torch.Tensor) or lists.dtype != torch.uint8 or lists.dim() != 3 or \
                lists.shape[1] != n + 1 or lists.device != self.device or lists.stride(2) != 1 or \
                lists.shape[2] < count:
            raise QbaError("lists must be a uint8 [n_inst, n+1, >= count] device tensor with unit column stride")
        call("qba_noise_profile_apply", self.ctx, n, _u64(seed_base), lists.shape[0], count, rates, n_rates, depol,
             _ptr(lists), lists.stride(1), lists.stride(0), self.stream())
        return lists

    # -- a grid of scenarios per checkpoint in one pass (qba_montecarlo_sweep_*) ----
    SWEEP_MAX = 16  # QBA_MC_SWEEP_MAX

    @classmethod
    def _check_sweep(cls, n: int, n_inst: int, counts, scenarios):
        """The argument check of the two montecarlo_sweep_* methods: the
        checkpoints as a list of ints and the scenarios as a list of
        ``(n_dishonest, word)``."""
        cs = cls._check_curve(n, 0, n_inst, counts)
        try:
            sc = [(int(k), word) for k, word in scenarios]
        except (TypeError, ValueError):
            raise QbaError("scenarios must be a sequence of (n_dishonest, policy word) pairs") from None
        if not 1 <= len(sc) <= cls.SWEEP_MAX:
            raise QbaError(f"between 1 and {cls.SWEEP_MAX} scenarios, not {len(sc)}")
        if len(cs) * len(sc) > cls.CURVE_MAX:
            raise QbaError(f"len(counts) * len(scenarios) must be <= {cls.CURVE_MAX}, not {len(cs) * len(sc)}")
        for i, (k, word) in enumerate(sc):
            if not 0 <= k <= n:
                raise QbaError(f"scenario {i}: n_dishonest={k} outside [0, {n}]")
            sc[i] = (k, cls._check_adversary(word))
            if sc[i][1] is None:
                raise QbaError(f"scenario {i}: the policy word is None (0xF is the reference's traitor)")
        return cs, sc

    @staticmethod
    def _scen_array(sc):
        return (Scenario * len(sc))(*(Scenario(k, word) for k, word in sc))

    def montecarlo_sweep_sampled(self, n: int, seed_base: int, n_inst: int, counts, scenarios,
                                 out: Optional[torch.Tensor] = None, flip_q16: int = 0) -> torch.Tensor:
        """The n_inst instances of montecarlo_curve_sampled decided at every
        count of ``counts`` under every scenario ``(n_dishonest, word)`` of
        ``scenarios`` (at most 16, and at most 32 slices in all) in one pass
        over their entries (qba_montecarlo_sweep_sampled): int32 [len(counts),
        len(scenarios), n_inst, 4 + 5*(n+1)], slice (j, s) word for word
        montecarlo_curve_sampled(..., adversary=word)[j] with that n_dishonest.
        ``flip_q16`` as there."""
        self._check_n(n)
        cs, sc = self._check_sweep(n, n_inst, counts, scenarios)
        flip = self._check_flip(flip_q16)
        self.prepare(n)
        out = self._sweep_out(n, n_inst, out, len(cs), len(sc))
        call("qba_montecarlo_sweep_sampled", self.ctx, n, _u64(seed_base), n_inst, (C.c_uint32 * len(cs))(*cs),
             len(cs), self._scen_array(sc), len(sc), flip, _ptr(out), self.stream())
        return out

    def montecarlo_sweep_lists(self, n: int, seed_base: int, lists, counts, scenarios,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_sweep_lists), as
        montecarlo_curve_lists takes them: slice (j, s) is
        montecarlo_curve_lists(..., adversary=word)[j] with that n_dishonest."""
        self._check_n(n)
        cs, sc = self._check_sweep(n, 0, counts, scenarios)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._sweep_out(n, n_inst, out, len(cs), len(sc))
        call("qba_montecarlo_sweep_lists", self.ctx, n, _u64(seed_base), n_inst, (C.c_uint32 * len(cs))(*cs),
             len(cs), self._scen_array(sc), len(sc), _ptr(lists), ld, stride, _ptr(out), self.stream())
        return out

    def _sweep_out(self, n: int, n_inst: int, out: Optional[torch.Tensor], k: int, s: int) -> torch.Tensor:
        """``out`` as [k, s, n_inst, words], or a new buffer when it is None; a
        contiguous [k * s, n_inst, words] buffer (the slices as
        montecarlo_tally takes them) is taken as well."""
        words = 4 + 5 * (n + 1)
        if isinstance(out, torch.Tensor) and out.is_contiguous() and tuple(out.shape) == (k, s, n_inst, words):
            out = out.view(k * s, n_inst, words)
        return self._rows_out(n, n_inst, out, k * s).view(k, s, n_inst, words)

    # -- a grid of (traitors, policy, network) scenarios in one pass (qba_montecarlo_grid_*) --
    GRID_MAX = 16  # QBA_MC_GRID_MAX

    @classmethod
    def _check_grid(cls, n: int, n_inst: int, counts, scenarios):
        """The argument check of the two montecarlo_grid_* methods: the
        checkpoints as a list of ints and the scenarios as a list of
        ``(n_dishonest, word, net)``."""
        cs = cls._check_curve(n, 0, n_inst, counts)
        try:
            sc = [(int(k), word, net) for k, word, net in scenarios]
        except (TypeError, ValueError):
            raise QbaError("scenarios must be a sequence of (n_dishonest, policy word, network word) triples") from None
        if not 1 <= len(sc) <= cls.GRID_MAX:
            raise QbaError(f"between 1 and {cls.GRID_MAX} scenarios, not {len(sc)}")
        if len(cs) * len(sc) > cls.CURVE_MAX:
            raise QbaError(f"len(counts) * len(scenarios) must be <= {cls.CURVE_MAX}, not {len(cs) * len(sc)}")
        for i, (k, word, net) in enumerate(sc):
            if not 0 <= k <= n:
                raise QbaError(f"scenario {i}: n_dishonest={k} outside [0, {n}]")
            if word is None:
                raise QbaError(f"scenario {i}: the policy word is None (0xF is the reference's traitor)")
            try:
                sc[i] = (k, cls._check_adversary(word), cls._check_net(net))
            except QbaError as e:
                raise QbaError(f"scenario {i}: {e}") from None
        return cs, sc

    @staticmethod
    def _grid_array(sc):
        return (GridScenario * len(sc))(*(GridScenario(k, word, net) for k, word, net in sc))

    def montecarlo_grid_sampled(self, n: int, seed_base: int, n_inst: int, counts, scenarios,
                                out: Optional[torch.Tensor] = None, flip_q16: int = 0) -> torch.Tensor:
        """The n_inst instances of montecarlo_curve_sampled_net decided at every
        count of ``counts`` under every scenario ``(n_dishonest, word, net)`` of
        ``scenarios`` (at most 16, and at most 32 slices in all) in one pass
        over their entries (qba_montecarlo_grid_sampled): int32 [len(counts),
        len(scenarios), n_inst, 4 + 5*(n+1)], slice (j, s) word for word
        montecarlo_curve_sampled_net(..., adversary=word, net=net)[j] with that
        n_dishonest.  ``flip_q16`` as there."""
        self._check_n(n)
        cs, sc = self._check_grid(n, n_inst, counts, scenarios)
        flip = self._check_flip(flip_q16)
        self.prepare(n)
        out = self._sweep_out(n, n_inst, out, len(cs), len(sc))
        call("qba_montecarlo_grid_sampled", self.ctx, n, _u64(seed_base), n_inst, (C.c_uint32 * len(cs))(*cs),
             len(cs), self._grid_array(sc), len(sc), flip, _ptr(out), self.stream())
        return out

    def montecarlo_grid_lists(self, n: int, seed_base: int, lists, counts, scenarios,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same from injected lists (qba_montecarlo_grid_lists), as
        montecarlo_curve_lists takes them: slice (j, s) is
        montecarlo_curve_lists_net(..., adversary=word, net=net)[j] with that
        n_dishonest."""
        self._check_n(n)
        cs, sc = self._check_grid(n, 0, counts, scenarios)
        lists, n_inst, ld, stride = self._mc_lists(n, lists, cs[-1])
        out = self._sweep_out(n, n_inst, out, len(cs), len(sc))
        call("qba_montecarlo_grid_lists", self.ctx, n, _u64(seed_base), n_inst, (C.c_uint32 * len(cs))(*cs),
             len(cs), self._grid_array(sc), len(sc), _ptr(lists), ld, stride, _ptr(out), self.stream())
        return out

    @classmethod
    def montecarlo_curve_shape(cls, n: int) -> Tuple[int, int, int]:
        """(wavefronts per workgroup, dynamic LDS bytes of a workgroup,
        workgroups per CU) of montecarlo_curve_sampled's kernel for the standard
        programs (qba_montecarlo_curve_shape); needs no device."""
        cls._check_n(n)
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        call("qba_montecarlo_curve_shape", n, C.byref(waves), C.byref(lds), C.byref(wgs))
        return waves.value, lds.value, wgs.value

    def montecarlo_program_shape(self, n: int, curve: bool = False) -> dict:
        """The launch shape of the program compiled for n on this engine right
        now (qba_montecarlo_program_shape): ``sampler`` (0 general, 1 canonical
        tables, 2 closed form), ``waves_compiled`` and ``waves_run`` per
        workgroup, ``lds_bytes`` of a workgroup and ``wgs_per_cu``, for
        montecarlo_sampled or (``curve``) montecarlo_curve_sampled.  Launches
        nothing."""
        self._check_n(n)
        samp, nw, run, lds, wgs = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        call("qba_montecarlo_program_shape", self.ctx, n, int(bool(curve)), C.byref(samp), C.byref(nw), C.byref(run),
             C.byref(lds), C.byref(wgs))
        return {"sampler": samp.value, "waves_compiled": nw.value, "waves_run": run.value, "lds_bytes": lds.value,
                "wgs_per_cu": wgs.value}

    # -- result rows reduced on the device (qba_montecarlo_tally) -------------------
    TALLY_WORDS = 32  # QBA_MC_TALLY_WORDS

    def montecarlo_tally(self, n: int, rows: torch.Tensor, tally: Optional[torch.Tensor] = None, inst_base: int = 0,
                         select: int = 0, capture: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Adds the result rows ``rows`` -- int32 [n_inst, 4 + 5*(n+1)] of a
        single-count call or [K, n_inst, ...] of a curve call -- to ``tally``,
        int64 [K, 32] (a zeroed one is allocated when None), and returns it;
        the words are montecarlo.T_*.  With ``select`` (montecarlo.SEL_* or-ed)
        the global indices ``inst_base + i`` of the matching rows of slice j go
        to ``capture[j]``, int64 [K, cap], at the slots word T_CAPTURE counts.
        Nothing is cleared, so calls accumulate.  Asynchronous."""
        self._check_n(n)
        words = 4 + 5 * (n + 1)
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() not in (2, 3) or \
                rows.shape[-1] != words or not rows.is_contiguous() or rows.device != self.device:
            raise QbaError(f"rows must be a contiguous int32 [n_inst, {words}] or [K, n_inst, {words}] device tensor")
        k, n_inst = (1, rows.shape[0]) if rows.dim() == 2 else (rows.shape[0], rows.shape[1])
        if not 1 <= k <= self.CURVE_MAX:
            raise QbaError(f"between 1 and {self.CURVE_MAX} slices, not {k}")
        if not 0 <= int(select) <= 7:
            raise QbaError("select is an or of montecarlo.SEL_FAILED, SEL_EMPTY_VI and SEL_STATUS")
        if tally is None:
            tally = torch.zeros((k, self.TALLY_WORDS), dtype=torch.int64, device=self.device)
        if not isinstance(tally, torch.Tensor) or tally.dtype != torch.int64 or \
                tuple(tally.shape) != (k, self.TALLY_WORDS) or not tally.is_contiguous() or tally.device != self.device:
            raise QbaError(f"tally must be a contiguous int64 [{k}, {self.TALLY_WORDS}] device tensor")
        cap = 0
        if capture is not None:
            if not isinstance(capture, torch.Tensor) or capture.dtype != torch.int64 or capture.dim() != 2 or \
                    capture.shape[0] != k or not capture.is_contiguous() or capture.device != self.device:
                raise QbaError(f"capture must be a contiguous int64 [{k}, cap] device tensor")
            cap = capture.shape[1]
        call("qba_montecarlo_tally", self.ctx, n, _ptr(rows), n_inst, k, _u64(inst_base), _ptr(tally),
             int(select), _ptr(capture) if cap else None, cap, self.stream())
        return tally

    # -- a transcript of chosen runs (qba_montecarlo_trace_*) --
    TRACE_CAP_MAX = 4096  # QBA_TRACE_CAP_MAX

    def _trace_args(self, n: int, n_dishonest: int, indices, count: int, flip_q16: int, adversary, cap: int,
                    n_match, out):
        """The checks the two montecarlo_trace_* methods share: ``(idx, n_idx,
        n_match, flip, word, (rows, counts, events))`` with the three outputs
        allocated when ``out`` is None."""
        self._check_n(n)
        self._check_curve(n, n_dishonest, 0, [count])
        flip = self._check_flip(flip_q16)
        adv = self._check_adversary(0xF if adversary is None else adversary)
        if not 1 <= int(cap) <= self.TRACE_CAP_MAX:
            raise QbaError(f"cap must be in [1, {self.TRACE_CAP_MAX}]")
        if not isinstance(indices, torch.Tensor):  # host indices: reduced mod 2^64 into the int64 the kernel adds
            host = np.array([int(i) & (2**64 - 1) for i in indices], dtype=np.uint64).view(np.int64)
            indices = torch.from_numpy(host).to(self.device)
        if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous() or \
                indices.device != self.device:
            raise QbaError("indices must be a contiguous int64 [n_idx] device tensor (or host integers)")
        if n_match is not None and (not isinstance(n_match, torch.Tensor) or n_match.dtype != torch.int64 or
                                    n_match.numel() != 1 or n_match.device != self.device):
            raise QbaError("n_match must be a one-element int64 device tensor")
        n_idx, g = indices.shape[0], n + 1
        shapes = ((n_idx, 4 + 5 * g), (n_idx, g), (n_idx, g, int(cap), 2))
        if out is None:
            out = tuple(torch.zeros(s, dtype=torch.int32, device=self.device) for s in shapes)
        if len(out) != 3 or any(not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != s or
                                not t.is_contiguous() or t.device != self.device for t, s in zip(out, shapes)):
            raise QbaError(f"out must be three contiguous int32 device tensors of shapes {shapes}")
        return indices, n_idx, n_match, flip, adv, tuple(out)

    def montecarlo_trace_sampled(self, n: int, n_dishonest: int, seed_base: int, indices, count: int, cap: int = 256,
                                 flip_q16: int = 0, adversary: Optional[int] = None,
                                 n_match: Optional[torch.Tensor] = None, out=None):
        """Re-run the instances keyed ``seed_base + indices[j]`` of
        montecarlo_sampled(..., flip_q16=, adversary=) with a transcript of
        their rounds (qba_montecarlo_trace_sampled): ``(rows, counts, events)``,
        int32 [n_idx, 4 + 5*(n+1)], [n_idx, n+1] and [n_idx, n+1, cap, 2] --
        the row of that key, how many events each rank produced, and the first
        ``cap`` of them as {head, pkt} bit patterns (montecarlo.EV_*,
        montecarlo.format_trace).  ``indices``: an int64 device tensor -- a
        tally's capture row as it lies -- or host integers.  ``n_match``: a
        one-element int64 device tensor (a tally's word T_CAPTURE); slots from
        ``min(n_idx, n_match)`` on are left untouched.  ``out``: the three
        tensors to write (new zeroed ones when None)."""
        idx, n_idx, n_match, flip, adv, out = self._trace_args(n, n_dishonest, indices, count, flip_q16, adversary,
                                                               cap, n_match, out)
        self.prepare(n)
        call("qba_montecarlo_trace_sampled", self.ctx, n, _u64(seed_base), _ptr(idx), n_idx,
             None if n_match is None else _ptr(n_match), count, n_dishonest, adv, flip, int(cap), _ptr(out[0]),
             _ptr(out[1]), _ptr(out[2]), self.stream())
        return out

    def montecarlo_trace_lists(self, n: int, n_dishonest: int, seed_base: int, indices, lists, count: int,
                               cap: int = 256, flip_q16: int = 0, adversary: Optional[int] = None,
                               n_match: Optional[torch.Tensor] = None, out=None):
        """The same from injected lists (qba_montecarlo_trace_lists), uint8
        [n_idx, n+1, >= count] as montecarlo_lists takes them: ``lists[j]``
        belongs to ``indices[j]``."""
        idx, n_idx, n_match, flip, adv, out = self._trace_args(n, n_dishonest, indices, count, flip_q16, adversary,
                                                               cap, n_match, out)
        lists, n_lists, ld, stride = self._mc_lists(n, lists, count)
        if n_lists != n_idx:
            raise QbaError(f"lists holds {n_lists} instances for {n_idx} indices")
        call("qba_montecarlo_trace_lists", self.ctx, n, _u64(seed_base), _ptr(idx), n_idx,
             None if n_match is None else _ptr(n_match), count, n_dishonest, adv, flip, int(cap), _ptr(lists), ld,
             stride, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), self.stream())
        return out

    # -- ... on a network that loses packets (qba_montecarlo_trace_*_net, section 13.13) --
    def montecarlo_trace_sampled_net(self, n: int, n_dishonest: int, seed_base: int, indices, count: int,
                                     cap: int = 256, flip_q16: int = 0, adversary: Optional[int] = None,
                                     n_match: Optional[torch.Tensor] = None, out=None, net: Optional[int] = None):
        """montecarlo_trace_sampled on lossy links
        (qba_montecarlo_trace_sampled_net): the same three outputs, the rows of
        montecarlo_curve_sampled_net at the one checkpoint ``count`` and the
        events with montecarlo.EV_SLOT_LOST and montecarlo.EV_NO_PACKET among
        them.  ``net``: the network word (montecarlo.net; None or 0: the perfect
        network, the outputs of montecarlo_trace_sampled)."""
        idx, n_idx, n_match, flip, adv, out = self._trace_args(n, n_dishonest, indices, count, flip_q16, adversary,
                                                               cap, n_match, out)
        word = self._check_net(net)
        self.prepare(n)
        call("qba_montecarlo_trace_sampled_net", self.ctx, n, _u64(seed_base), _ptr(idx), n_idx,
             None if n_match is None else _ptr(n_match), count, n_dishonest, adv, flip, int(cap), _ptr(out[0]),
             _ptr(out[1]), _ptr(out[2]), self.stream(), word)
        return out

    def montecarlo_trace_lists_net(self, n: int, n_dishonest: int, seed_base: int, indices, lists, count: int,
                                   cap: int = 256, flip_q16: int = 0, adversary: Optional[int] = None,
                                   n_match: Optional[torch.Tensor] = None, out=None, net: Optional[int] = None):
        """The same from injected lists (qba_montecarlo_trace_lists_net), as
        montecarlo_trace_lists takes them."""
        idx, n_idx, n_match, flip, adv, out = self._trace_args(n, n_dishonest, indices, count, flip_q16, adversary,
                                                               cap, n_match, out)
        word = self._check_net(net)
        lists, n_lists, ld, stride = self._mc_lists(n, lists, count)
        if n_lists != n_idx:
            raise QbaError(f"lists holds {n_lists} instances for {n_idx} indices")
        call("qba_montecarlo_trace_lists_net", self.ctx, n, _u64(seed_base), _ptr(idx), n_idx,
             None if n_match is None else _ptr(n_match), count, n_dishonest, adv, flip, int(cap), _ptr(lists), ld,
             stride, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), self.stream(), word)
        return out

    # -- (A5-A8) count mode -------------------------------------------------------
    def check_counts(self, lists: torch.Tensor, n: int, count: int,
                     counts: Optional[Counts] = None, accumulate: bool = False) -> Counts:
        self._check_n(n)
        if counts is None:
            counts = self.alloc_counts(n)
        ld = self._lists_ok(lists, n, count)
        call("qba_check_counts", self.ctx, n, _ptr(lists), count, ld, _ptr(counts.H),
             _ptr(counts.C), _ptr(counts.P), int(accumulate), self.stream())
        return counts

    def check_counts_packed(self, packed: torch.Tensor, n: int, count: int,
                            counts: Optional[Counts] = None, accumulate: bool = False) -> Counts:
        self._check_n(n)
        if counts is None:
            counts = self.alloc_counts(n)
        ld = self._packed_ok(packed, n + 1, count)
        call("qba_check_counts_packed", self.ctx, n, _ptr(packed), count, ld, _ptr(counts.H),
             _ptr(counts.C), _ptr(counts.P), int(accumulate), self.stream())
        return counts

    def pack(self, lists: torch.Tensor, rows: int, count: int,
             packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Byte rows -> nibble rows on the device; raises when a value > 15."""
        if lists.dtype != torch.uint8 or lists.dim() != 2 or lists.shape[0] < rows or \
                lists.stride(1) != 1 or lists.shape[1] < count:
            raise QbaError("lists must be a uint8 [>= rows, >= count] device tensor")
        if packed is None:
            packed = torch.empty((rows, _row_ld((count + 1) // 2)), dtype=torch.uint8, device=self.device)
        ldp = self._packed_ok(packed, rows, count)
        bad = torch.empty(1, dtype=torch.int64, device=self.device)
        call("qba_lists_pack", self.ctx, _ptr(lists), lists.stride(0), rows, count, _ptr(packed), ldp,
             _ptr(bad), self.stream())
        if int(bad.item()):
            raise QbaError(f"{int(bad.item())} values > 15 cannot be stored as nibbles")
        return packed

    def unpack(self, packed: torch.Tensor, rows: int, count: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Nibble rows -> byte rows [rows, ld] on the device."""
        ldp = self._packed_ok(packed, rows, count)
        if out is None:
            out = torch.empty((rows, _row_ld(count)), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < rows or out.stride(1) != 1 or \
                out.shape[1] < count:
            raise QbaError("out must be a uint8 [>= rows, >= count] device tensor")
        call("qba_lists_unpack", self.ctx, _ptr(packed), ldp, rows, count, _ptr(out), out.stride(0),
             self.stream())
        return out

    def count_tables(self, n: int, sizeL: int, seed: int = 0, lists: Optional[np.ndarray] = None,
                     chunk: int = 1 << 27, first: int = 0, device_out: bool = False):
        """Flat int64 [H | C | P] over entries [first, first + sizeL): injected
        host lists (shape (n+1, sizeL)) are checked on the device, otherwise
        entries are sampled and checked in chunks of `chunk` (lists are written
        once to a reused buffer).  device_out returns the device tensor (for a
        collective) instead of a host copy."""
        self._check_n(n)
        _, w = self.sizes(n)
        g = n + 1
        h, c = w * g * w, w * g * g
        flat = torch.zeros(h + c + w, dtype=torch.int64, device=self.device)
        counts = Counts(flat[:h].view(w, g, w), flat[h:h + c].view(w, g, g), flat[h + c:])
        if lists is not None:
            arr = np.ascontiguousarray(lists, dtype=np.uint8)
            if arr.shape != (g, sizeL):
                raise QbaError(f"lists must have shape {(g, sizeL)}")
            dev = self.alloc_lists(n, sizeL)
            dev[:, :sizeL] = torch.from_numpy(arr).to(self.device)
            self.check_counts(dev, n, sizeL, counts)
        else:
            # the lists are sampled, counted and dropped: nibble rows (half the
            # bytes written)
            chunk = max(8, chunk & ~7)
            buf = self.alloc_packed(n, min(chunk, max(sizeL, 1)))
            for off in range(0, sizeL, chunk):
                self.sample_check_packed(n, seed, first + off, min(chunk, sizeL - off), buf, counts,
                                         accumulate=off > 0)
        if sizeL and self.last_stats()[0] != 0:
            raise QbaError("lists hold values >= w at Q-correlated positions: count mode "
                           "cannot evaluate them (the reference never produces such lists)")
        return flat if device_out else flat.cpu().numpy()

    def last_stats(self) -> np.ndarray:
        out = np.zeros(2, np.int64)
        call("qba_last_stats", self.ctx, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return out

    def reserve(self, n: int, max_blocks: int) -> None:
        call("qba_reserve", self.ctx, n, max_blocks)

    # -- (A5-A8) exact-order mode -----------------------------------------------
    def to_device(self, arr) -> torch.Tensor:
        return torch.as_tensor(np.ascontiguousarray(arr)).to(self.device, non_blocking=False)

    @staticmethod
    def to_host(t: torch.Tensor) -> np.ndarray:
        return t.cpu().numpy()

    def isq_indices(self, li: torch.Tensor, lc: torch.Tensor) -> np.ndarray:
        """Ascending {k : Li[k] != Lc[k]} (tfg.py:327)."""
        count = li.numel()
        out = np.empty(max(count, 1), np.int64)
        found = C.c_int64()
        call("qba_isq_indices_host", self.ctx, _ptr(li), _ptr(lc), count, out.ctypes.data, count,
             C.byref(found), self.stream())
        return out[: found.value]

    def select_eq(self, order: np.ndarray, lc: torch.Tensor, v: int) -> np.ndarray:
        """[x for x in order if Lc[x] == v], order kept (tfg.py:182)."""
        m = len(order)
        if m == 0:
            return np.zeros(0, np.int64)
        h_order = np.ascontiguousarray(order, dtype=np.int64)
        out = np.empty(m, np.int64)
        found = C.c_int64()
        call("qba_select_eq_host", self.ctx, h_order.ctypes.data, m, _ptr(lc), lc.numel(), int(v),
             out.ctypes.data, C.byref(found), self.stream())
        return out[: found.value]

    def gather(self, li: torch.Tensor, order: np.ndarray) -> np.ndarray:
        """Li[j] for j in order (tfg.py:189, 291)."""
        m = len(order)
        if m == 0:
            return np.zeros(0, np.int64)
        d_idx = self.to_device(np.asarray(order, dtype=np.int64))
        out = torch.empty(m, dtype=torch.int64, device=self.device)
        call("qba_gather", self.ctx, _ptr(li), li.numel(), _ptr(d_idx), m, _ptr(out), self.stream())
        return out.cpu().numpy()

    def check_packet(self, li: torch.Tensor, order: np.ndarray, rows: Sequence[Sequence[int]], v: int,
                     w: int) -> Tuple[tuple, bool]:
        """One packet of the exact-order protocol (tfg.py:189-192, 291-294):
        own = tuple(Li[j] for j in order) and Cond2/Cond3 of
        consistent(v, rows | {own}, w), in one launch and one host sync
        (qba_check_packet_host).  All rows must have len(order) entries
        (Cond1 stays with the caller)."""
        ln, m = len(order), len(rows)
        stage = np.empty(ln * (m + 1), np.int64)
        _packet_stage(stage, 0, order, rows)
        o = np.empty(ln + 3 + m, np.int64)
        call("qba_check_packet_host", self.ctx, _ptr(li), li.numel(), stage.ctypes.data, m, ln, int(v), int(w),
             o.ctypes.data, self.stream())
        own, ok = _packet_result(o, 0, ln, m, "qba_check_packet")
        return tuple(own.tolist()), ok

    def check_packets(self, li: torch.Tensor, reqs: Sequence[Tuple[np.ndarray, Sequence, int]],
                      w: int) -> list:
        """A round's packets (tfg.py:337-348 -> 289-294) in one device round
        trip (qba_check_packets_host): reqs = [(order, rows, v)], each as
        :meth:`check_packet`; returns [(own, ok, own_wire)] in the same order
        (own_wire: the own tuple as the int64 array it travels as)."""
        if not reqs:
            return []
        dims = [(len(o), len(r)) for o, r, _ in reqs]
        stage = np.empty(max(sum(ln * (m + 1) for ln, m in dims), 1), np.int64)
        desc = np.empty(3 * len(reqs), np.int64)
        off = 0
        for i, ((order, rows, v), (ln, m)) in enumerate(zip(reqs, dims)):
            desc[3 * i:3 * i + 3] = (m, ln, int(v))
            off = _packet_stage(stage, off, order, rows)
        out = np.empty(sum(ln + 3 + m for ln, m in dims), np.int64)
        call("qba_check_packets_host", self.ctx, _ptr(li), li.numel(), stage.ctypes.data, desc.ctypes.data,
             len(reqs), int(w), out.ctypes.data, self.stream())
        res, o = [], 0
        for ln, m in dims:
            own, ok = _packet_result(out, o, ln, m, "qba_check_packets_host")
            res.append((tuple(own.tolist()), ok, own))
            o += ln + 3 + m
        return res

    def check_gather(self, lists: torch.Tensor, count: int, idx: np.ndarray, party: Sequence[int], v: int,
                     w: int) -> bool:
        """consistent(v, L, w) (tfg.py:87-98) over the tuples
        L = {tuple(lists[party[a]][j] for j in idx[a])}, gathered and checked on
        the device (qba_check_gather; identical tuples collapse as in the
        reference's set).  idx: int64 [m, len]."""
        idx_d = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64), device=self.device)
        m = idx_d.shape[0]
        ln = idx_d.shape[1] if idx_d.dim() == 2 else 0
        party_d = torch.as_tensor(np.asarray(party, dtype=np.int32), device=self.device)
        ok = torch.empty(1, dtype=torch.int32, device=self.device)
        call("qba_check_gather", self.ctx, _ptr(lists), lists.stride(0), lists.shape[0], count, _ptr(idx_d),
             _ptr(party_d), m, ln, int(v), int(w), _ptr(ok), self.stream())
        r = int(ok.item())
        if r < 0:
            raise QbaError("qba_check_gather: index or party outside the lists")
        return bool(r)

    def lists_to_bits(self, lists: torch.Tensor, rows: int, count: int, nq: int) -> np.ndarray:
        """rawS (tfg.py:81-84): rows [0, rows) encoded, host int64 [rows, count*nq]."""
        out = np.empty((rows, count * nq), np.int64)
        call("qba_lists_to_bits_host", self.ctx, _ptr(lists), lists.stride(0), rows, count, nq,
             out.ctypes.data, self.stream())
        return out

    def bits_to_values_host(self, raw: np.ndarray, count: int, nq: int) -> torch.Tensor:
        """measure_to_ints (tfg.py:158, 161) of a received host buffer -> device list."""
        raw = np.ascontiguousarray(raw, dtype=np.int64)
        out = torch.empty(max(count, 1), dtype=torch.uint8, device=self.device)
        call("qba_bits_to_values_host", self.ctx, raw.ctypes.data, count, nq, _ptr(out), self.stream())
        return out[:count]

    def allreduce_i64(self, t: torch.Tensor) -> torch.Tensor:
        """In-place sum over the RCCL communicator of rccl_init (qba_allreduce_i64)."""
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != self.device:
            raise QbaError("allreduce_i64 needs a contiguous int64 tensor on this engine's device")
        call("qba_allreduce_i64", self.ctx, _ptr(t), t.numel(), self.stream())
        return t

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        call("qba_rccl_unique_id", buf)
        return bytes(buf)

    def rccl_init(self, uid: bytes, nranks: int, rank: int) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        call("qba_rccl_init", self.ctx, buf, nranks, rank)

    def consistent_rows(self, rows: np.ndarray, v: int, w: int) -> bool:
        """Cond2 and Cond3 of tfg.py:93-98 over an (m, len) int64 matrix."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        m, ln = rows.shape
        d = self.to_device(rows) if ln > 0 else torch.zeros(1, dtype=torch.int64, device=self.device)
        ok = C.c_int32()
        call("qba_consistent", self.ctx, _ptr(d), m, ln, int(v), int(w), C.byref(ok), self.stream())
        return bool(ok.value)

    # -- codec (rawS wire layout) ----------------------------------------------
    def bits_to_values(self, raw: torch.Tensor, count: int, nq: int) -> torch.Tensor:
        out = torch.empty(max(count, 1), dtype=torch.uint8, device=self.device)
        call("qba_bits_to_values", self.ctx, _ptr(raw), count, nq, _ptr(out), self.stream())
        return out[:count]

    def values_to_bits(self, values: torch.Tensor, count: int, nq: int) -> torch.Tensor:
        out = torch.empty(max(count * nq, 1), dtype=torch.int64, device=self.device)
        call("qba_values_to_bits", self.ctx, _ptr(values), count, nq, _ptr(out), self.stream())
        return out[: count * nq]

    # -- statevector -------------------------------------------------------------
    def statevector(self, nqubits: int, gates: np.ndarray,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        sv = out if out is not None else torch.empty(1 << nqubits, dtype=torch.float64, device=self.device)
        g = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
        call("qba_sv_prepare", self.ctx, _ptr(sv), nqubits, _i32p(g), len(g), self.stream())
        return sv

    def statevector_unfused(self, nqubits: int, gates: np.ndarray,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """qba_sv_init + qba_sv_apply: no folding of the single-qubit layer into
        the init pass (the H/X/CX run fusion of qba_sv_apply still applies)."""
        sv = out if out is not None else torch.empty(1 << nqubits, dtype=torch.float64, device=self.device)
        g = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
        call("qba_sv_init", self.ctx, _ptr(sv), nqubits, self.stream())
        call("qba_sv_apply", self.ctx, _ptr(sv), nqubits, _i32p(g), len(g), self.stream())
        return sv

    def apply_gates(self, sv: torch.Tensor, nqubits: int, gates: np.ndarray) -> None:
        g = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
        call("qba_sv_apply", self.ctx, _ptr(sv), nqubits, _i32p(g), len(g), self.stream())

    def support(self, sv: torch.Tensor, nqubits: int, eps: float = 1e-24,
                cap: int = 1 << 20) -> Tuple[np.ndarray, np.ndarray]:
        idx = torch.empty(cap, dtype=torch.int64, device=self.device)
        prob = torch.empty(cap, dtype=torch.float64, device=self.device)
        cnt = C.c_int64()
        call("qba_sv_support", self.ctx, _ptr(sv), nqubits, float(eps), _ptr(idx), _ptr(prob), cap,
             C.byref(cnt), self.stream())
        k = min(cnt.value, cap)
        if cnt.value > cap:
            raise QbaError(f"support of {cnt.value} outcomes exceeds cap={cap}")
        return idx[:k].cpu().numpy(), prob[:k].cpu().numpy()

    # -- test helpers -------------------------------------------------------------
    def set_test_knobs(self, chunk: int = 0, pb_min: int = -1, list_grid: int = 0) -> "Engine":
        """qba_test_set_knobs: launch-shape knobs for the GPU tests (0 / -1 / 0
        = the shipped selection).  Results never change, only which kernel
        path computes them."""
        call("qba_test_set_knobs", self.ctx, chunk, pb_min, list_grid)
        return self

    def philox(self, ctr: np.ndarray, key: int) -> np.ndarray:
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        d_ctr = self.to_device(ctr.view(np.int32))
        out = torch.empty_like(d_ctr)
        call("qba_philox_dev", self.ctx, _ptr(d_ctr), len(ctr), int(key), _ptr(out), self.stream())
        return out.cpu().numpy().view(np.uint32)


def unpack_nibbles(packed: np.ndarray, count: int) -> np.ndarray:
    """Host view of nibble rows [rows, >= (count+1)//2] as byte rows [rows, count]."""
    p = np.asarray(packed, dtype=np.uint8)
    out = np.empty((p.shape[0], 2 * ((count + 1) // 2)), dtype=np.uint8)
    out[:, 0::2] = p[:, :(count + 1) // 2] & 15
    out[:, 1::2] = p[:, :(count + 1) // 2] >> 4
    return out[:, :count]


def alias_build(probs: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """Host Vose alias table (exported for tests): (thr u64 in [0, 2^32], alias i32)."""
    p = np.ascontiguousarray(probs, dtype=np.float64)
    thr = np.zeros(len(p), np.uint64)
    alias = np.zeros(len(p), np.int32)
    call("qba_alias_build", p.ctypes.data_as(C.POINTER(C.c_double)), len(p),
         thr.ctypes.data_as(C.POINTER(C.c_uint64)), alias.ctypes.data_as(C.POINTER(C.c_int32)))
    return thr, alias
