"""Device context: owns one ``vrpms_ctx`` and moves instances/tours through the
C-ABI.  PyTorch-ROCm tensors are used only as device-buffer owners and for
the current HIP stream; all arithmetic happens in libvrpms's kernels.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (CVRP, INJECT_BETTER, INJECT_SORTED, INJECT_WORST, OBJ_MAX,  # noqa: F401
                   OBJ_SUM, TSP, VrpmsError, check)


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("vrpms_amd needs a ROCm GPU: torch.cuda.is_available() is False "
                           "(there is no CPU fallback by design)")
    return torch


def perm_dtype_bytes(t) -> int:
    torch = _torch()
    if t.dtype == torch.uint8:
        return 1
    if t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
        return 2
    raise TypeError(f"tours must be uint8 or (u)int16, got {t.dtype}")


def tour_dtype(N: int):
    """Narrowest tour element for an N-node instance (uint8 for N <= 256)."""
    torch = _torch()
    return torch.uint8 if N <= 256 else torch.int16


def _u64(seed) -> int:
    """A seed as the uint64 the C entry points take."""
    return int(seed) & (2**64 - 1)


def _bytes(symbol: str, *ints) -> int:
    """The library's size function `symbol` for those arguments: each takes
    ints and a uint64 to write the bytes to.  Host only."""
    nbytes = ctypes.c_uint64()
    check(getattr(_lib.load(), symbol)(*map(int, ints), ctypes.byref(nbytes)))
    return int(nbytes.value)


def vrp_batch_sp_lds(n: int, K: int, team: int = 0) -> int:
    """vrpms_vrp_batch_sp_lds: the dynamic-LDS bytes of a vrp_batch_sp launch
    for n customers, K vehicles and `team` threads per request (0 = the auto
    team).  Host only: needs the library, no GPU."""
    return _bytes("vrpms_vrp_batch_sp_lds", n, K, team)


def tsp_batch_tdp_lds(n: int, H: int, W: int, team: int = 0) -> int:
    """vrpms_tsp_batch_tdp_lds: the dynamic-LDS bytes of a tsp_batch_tdp
    launch for n customers, H hour slices (1 or 24), rows of W hour words and
    `team` threads per request (0 = the auto team).  Host only: needs the
    library, no GPU."""
    return _bytes("vrpms_tsp_batch_tdp_lds", n, H, W, team)


def vrp_batch_tdsp_lds(n: int, K: int, G: int, H: int, W: int, team: int = 0) -> int:
    """vrpms_vrp_batch_tdsp_lds: the dynamic-LDS bytes of a vrp_batch_tdsp
    launch for n customers, K vehicles, at most G distinct start times per
    request, H hour slices (1 or 24), rows of W hour words and `team` threads
    per request (0 = the auto team).  Host only: needs the library, no GPU."""
    return _bytes("vrpms_vrp_batch_tdsp_lds", n, K, G, H, W, team)


def vrp_batch_sa_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_sa_lds: the dynamic-LDS bytes of a vrp_batch_sa launch
    for N nodes, K vehicles, H hour slices (1 or 24) and a uint16 (`wide`
    false) or int32 (`wide` true) matrix.  Host only: needs the library, no
    GPU."""
    return _bytes("vrpms_vrp_batch_sa_lds", N, K, H, wide)


def vrp_batch_ga_lds(N: int, K: int, H: int, wide, P: int) -> int:
    """vrpms_vrp_batch_ga_lds: the dynamic-LDS bytes of a vrp_batch_ga launch
    for N nodes, K vehicles, H hour slices (1 or 24), a uint16 (`wide` false)
    or int32 (`wide` true) matrix and a population of P.  Host only: needs the
    library, no GPU."""
    return _bytes("vrpms_vrp_batch_ga_lds", N, K, H, wide, P)


def vrp_batch_aco_lds(N: int, K: int, H: int, wide, A: int) -> int:
    """vrpms_vrp_batch_aco_lds: the dynamic-LDS bytes of a vrp_batch_aco launch
    for N nodes, K vehicles, H hour slices (1 or 24), a uint16 (`wide` false)
    or int32 (`wide` true) matrix and A ants.  Host only: needs the library,
    no GPU."""
    return _bytes("vrpms_vrp_batch_aco_lds", N, K, H, wide, A)


def vrp_batch_ls_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_ls_lds: the dynamic-LDS bytes of a vrp_batch_ls launch
    for N nodes, K vehicles, H hour slices (1 or 24) and a uint16 (`wide`
    false) or int32 (`wide` true) matrix; never more than vrp_batch_sa_lds of
    the same shape.  Host only: needs the library, no GPU."""
    return _bytes("vrpms_vrp_batch_ls_lds", N, K, H, wide)


def tsp_batch_lso_lds(N: int, H: int, wide) -> int:
    """vrpms_tsp_batch_lso_lds: the dynamic-LDS bytes of a tsp_batch_lso launch
    for N nodes, H hour slices (1 or 24) and a uint16 (`wide` false) or int32
    (`wide` true) matrix.  Host only: needs the library, no GPU."""
    return _bytes("vrpms_tsp_batch_lso_lds", N, H, wide)


def tsp_batch_lso_spread_lds(N: int, H: int, wide) -> int:
    """vrpms_tsp_batch_lso_spread_lds: the dynamic-LDS bytes of the descents
    launch of tsp_batch_lso_spread for N nodes, H hour slices (1 or 24) and a
    uint16 (`wide` false) or int32 (`wide` true) matrix; never more than
    tsp_batch_lso_lds of the same shape.  Host only: needs the library, no
    GPU."""
    return _bytes("vrpms_tsp_batch_lso_spread_lds", N, H, wide)


def tsp_batch_lso_spread_work(R: int, N: int, G: int) -> int:
    """vrpms_tsp_batch_lso_spread_work: the workspace bytes of a
    tsp_batch_lso_spread launch of R requests at G workgroups each,
    R * G * (24 + 2 * align8(N - 1)).  Host only: needs the library, no GPU."""
    return _bytes("vrpms_tsp_batch_lso_spread_work", R, N, G)


def vrp_batch_lsr_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_lsr_lds: the dynamic-LDS bytes of a vrp_batch_lsr launch
    for N nodes, K vehicles, H hour slices (1 or 24) and a uint16 (`wide`
    false) or int32 (`wide` true) matrix; never more than vrp_batch_sa_lds of
    the same shape.  Host only: needs the library, no GPU."""
    return _bytes("vrpms_vrp_batch_lsr_lds", N, K, H, wide)


def vrp_batch_lsf_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_lsf_lds: the dynamic-LDS bytes of a vrp_batch_lsf launch
    for N nodes, K vehicles and a uint16 (`wide` false) or int32 (`wide` true)
    static matrix.  H is taken so that the call reads like the other _lds
    functions and must be 1.  Host only: needs the library, no GPU."""
    if int(H) != 1:
        raise ValueError(f"vrp_batch_lsf_lds: H must be 1 ({H} given): an hour-indexed matrix "
                         "keeps vrp_batch_lsr")
    return _bytes("vrpms_vrp_batch_lsf_lds", N, K, wide)


def vrp_batch_lsr_spread_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_lsr_spread_lds: the dynamic-LDS bytes of either launch
    of vrp_batch_lsr_spread for N nodes, K vehicles, H hour slices (1 or 24)
    and a uint16 (`wide` false) or int32 (`wide` true) matrix; never more than
    vrp_batch_lsr_lds of the same shape.  Host only: needs the library, no
    GPU."""
    return _bytes("vrpms_vrp_batch_lsr_spread_lds", N, K, H, wide)


def vrp_batch_lsr_spread_work(R: int, N: int, K: int, G: int) -> int:
    """vrpms_vrp_batch_lsr_spread_work: the workspace bytes of a
    vrp_batch_lsr_spread launch of R requests at G workgroups each,
    R * G * (16 + 2 * align8(N + K - 2)).  Host only: needs the library, no
    GPU."""
    return _bytes("vrpms_vrp_batch_lsr_spread_work", R, N, K, G)


def vrp_batch_lsf_spread_lds(N: int, K: int, H: int, wide) -> int:
    """vrpms_vrp_batch_lsf_spread_lds: the dynamic-LDS bytes of either launch
    of vrp_batch_lsf_spread for N nodes, K vehicles and a uint16 (`wide`
    false) or int32 (`wide` true) static matrix; never more than
    vrp_batch_lsf_lds of the same shape.  H is taken so that the call reads
    like the other _lds functions and must be 1.  Host only: needs the
    library, no GPU."""
    if int(H) != 1:
        raise ValueError(f"vrp_batch_lsf_spread_lds: H must be 1 ({H} given): an hour-indexed "
                         "matrix keeps vrp_batch_lsr_spread")
    return _bytes("vrpms_vrp_batch_lsf_spread_lds", N, K, wide)


def vrp_batch_lsf_spread_work(R: int, N: int, K: int, G: int) -> int:
    """vrpms_vrp_batch_lsf_spread_work: the workspace bytes of a
    vrp_batch_lsf_spread launch of R requests at G workgroups each,
    R * G * (16 + 2 * align8(N + K - 2)).  Host only: needs the library, no
    GPU."""
    return _bytes("vrpms_vrp_batch_lsf_spread_work", R, N, K, G)


def tdp_words(start: int, horizon: int) -> int:
    """Hour words of one A16 row: the words from the start's hour to the one
    of start + horizon."""
    return (int(start) % 60 + int(horizon)) // 60 + 1


class Context:
    """One solver context on one GPU (``vrpms_ctx_create``)."""

    def __init__(self, device: int = 0):
        torch = require_gpu()
        self.lib = _lib.load()
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        ptr = ctypes.c_void_p()
        check(self.lib.vrpms_ctx_create(self.device, ctypes.byref(ptr)))
        self._ctx = ptr
        self.problem = None
        self.N = self.H = self.K = 0
        self.start_times = []
        self.objective = OBJ_SUM
        # (group, world) once islands.init_comm agreed on a communicator
        self.island_comm_group = None

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.vrpms_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._ctx

    def stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.dev).cuda_stream)

    @property
    def cus(self) -> int:
        """The device's compute units."""
        return int(_torch().cuda.get_device_properties(self.dev).multi_processor_count)

    # -- instance -----------------------------------------------------------
    def set_instance(self, problem: int, durations, demand=None, capacities=None,
                     start_times=(0,), objective: int = OBJ_SUM):
        """``durations``: int [N][N] or [H][N][N] (compact node indices)."""
        torch = _torch()
        D = np.asarray(durations)
        if D.ndim == 2:
            D = D[None]
        if D.ndim != 3 or D.shape[1] != D.shape[2]:
            raise ValueError("durations must be [N][N] or [H][N][N]")
        if D.size and (D.min() < np.iinfo(np.int32).min or D.max() > np.iinfo(np.int32).max):
            raise VrpmsError(_lib.VRPMS_ERANGE, "durations do not fit int32")
        H, N = int(D.shape[0]), int(D.shape[1])
        st = np.asarray(start_times, dtype=np.int64).reshape(-1)
        K = int(st.shape[0])
        d_dur = torch.as_tensor(np.ascontiguousarray(D, dtype=np.int32), device=self.dev)
        d_st = torch.as_tensor(st.astype(np.int32), device=self.dev)
        d_dem = d_cap = None
        if problem == CVRP:
            d_dem = torch.as_tensor(np.asarray(demand, dtype=np.int32).reshape(-1), device=self.dev)
            d_cap = torch.as_tensor(np.asarray(capacities, dtype=np.int32).reshape(-1), device=self.dev)
            if d_dem.numel() != N:
                raise ValueError(f"demand has {d_dem.numel()} entries, matrix has {N} nodes")
            if d_cap.numel() != K:
                raise ValueError("capacities and start_times must have the same length")
        check(self.lib.vrpms_set_instance(
            self._ctx, int(problem), d_dur.data_ptr(), H, N,
            d_dem.data_ptr() if d_dem is not None else None,
            d_cap.data_ptr() if d_cap is not None else None,
            d_st.data_ptr(), K, int(objective), self.stream()))
        self.problem, self.N, self.H, self.K, self.objective = problem, N, H, K, objective
        self.start_times = [int(t) for t in st]

    # -- scoring ------------------------------------------------------------
    def eval(self, perms, n: int | None = None, with_parts: bool = False, out=None):
        """Score a [C][ld] tour tensor on the device.  Returns keys (uint64
        stored as int64) or (keys, sums, maxs, unvisited) with ``with_parts``."""
        torch = _torch()
        if perms.device != self.dev or perms.dim() != 2:
            raise ValueError(f"tours must be a 2-D tensor on {self.dev}")
        if not perms.is_contiguous():
            raise ValueError("tours must be contiguous")
        C, ld = perms.shape
        n = ld if n is None else int(n)
        pb = perm_dtype_bytes(perms)
        keys = out if out is not None else torch.empty(C, dtype=torch.int64, device=self.dev)
        sums = maxs = unv = None
        if with_parts:
            sums = torch.empty(C, dtype=torch.int32, device=self.dev)
            maxs = torch.empty(C, dtype=torch.int32, device=self.dev)
            unv = torch.empty(C, dtype=torch.int32, device=self.dev)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        check(self.lib.vrpms_eval(self._ctx, perms.data_ptr(), pb, C, n, ld, keys.data_ptr(),
                                  ptr(sums), ptr(maxs), ptr(unv), self.stream()))
        return (keys, sums, maxs, unv) if with_parts else keys

    def to_words(self, perms, n: int | None = None):
        """uint8 [C][ld] rows -> int32 [ceil(n/4)][C] word-interleaved layout."""
        torch = _torch()
        C, ld = perms.shape
        n = ld if n is None else int(n)
        words = torch.empty(((n + 3) // 4, C), dtype=torch.int32, device=self.dev)
        check(self.lib.vrpms_rows_to_words(self._ctx, perms.data_ptr(), C, n, ld,
                                           words.data_ptr(), self.stream()))
        return words

    def eval_words(self, words, n: int, with_parts: bool = False, out=None):
        """Score tours in the word-interleaved layout (see vrpms_eval_words)."""
        torch = _torch()
        if words.device != self.dev or words.dim() != 2 or not words.is_contiguous():
            raise ValueError("words must be a contiguous 2-D tensor on the context device")
        if words.shape[0] != (int(n) + 3) // 4:
            raise ValueError("words must have ceil(n/4) rows")
        C = words.shape[1]
        keys = out if out is not None else torch.empty(C, dtype=torch.int64, device=self.dev)
        parts = [torch.empty(C, dtype=torch.int32, device=self.dev) for _ in range(3)] \
            if with_parts else [None, None, None]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        check(self.lib.vrpms_eval_words(self._ctx, words.data_ptr(), C, int(n), keys.data_ptr(),
                                        *[ptr(p) for p in parts], self.stream()))
        return (keys, *parts) if with_parts else keys

    def set_split_mode(self, mode: int):
        """0 = auto (branch-free prefix-ret split when it fits), 2 = branchy."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_SPLIT_MODE, int(mode)))

    def set_words_kernel(self, gen: int):
        """Path 0 of vrpms_eval: 0 = auto (eval_cvrp_rows2), 1 = eval_cvrp_packed."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_WORDS_KERNEL, int(gen)))

    def set_sa_route(self, mode: int):
        """0 = auto (O(1) segment pricing on static symmetric instances,
        hour-row walks on hour-indexed ones, else route-local walks for
        windowed SA), 2 = full re-evaluation (sa_kernel), 3 = force the
        route-local walks, 4 = force the hour-row walks (sa_td_kernel)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_SA_ROUTE, int(mode)))

    def set_route_wg_per_cu(self, wg: int):
        """sa_route_kernel workgroups per CU: 0 = auto (1 for multi-wavefront
        chains), 1 or 2 force."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_ROUTE_WG_PER_CU, int(wg)))

    def set_seg_waves(self, w: int):
        """sa_seg_kernel wavefronts per chain: 0 = auto, 1..4 force (A/B)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_SEG_WAVES, int(w)))

    def set_aco_construct(self, mode: int):
        """0 = auto (LDS-staged colony weights when they fit), 2 = the L2 path (A/B)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_ACO_CONSTRUCT, int(mode)))

    def set_ga_fused(self, mode: int):
        """0 = auto (fused one-workgroup-per-island GA when it fits), 2 = three kernels."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_GA_FUSED, int(mode)))

    def set_rows_config(self, cfg: int):
        """eval_cvrp_rows2 (CW, ILP): 0 = auto, 1 = (8, 2), 2 = (16, 1),
        3 = (4, 2), 4 = (8, 1), 5 = (4, 1)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_ROWS_CONFIG, int(cfg)))

    def set_words_ilp(self, ilp: int):
        """Candidates per lane in eval_cvrp_words2: 0 = auto, 1 or 2 force."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_WORDS_ILP, int(ilp)))

    def set_words_lookahead(self, la: int):
        """Words of gathers eval_cvrp_words2 keeps in flight: 0 = auto, 1 or 2."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_WORDS_LOOKAHEAD, int(la)))

    def set_staged_m(self, m: int):
        """Candidates per lane in eval_staged: 0 = auto, 1 or 2 force."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_STAGED_M, int(m)))

    def eval_path(self, perms) -> int:
        return self.lib.vrpms_eval_path(self._ctx, perm_dtype_bytes(perms), perms.shape[-1],
                                        perms.data_ptr())

    LAYOUT_FIELDS = ("use16", "tier", "pack_w", "pref_S", "pref_lim", "uniform_cap", "symmetric",
                     "sym_all", "flex", "fast", "ks", "B", "carry", "hour_minor")

    def instance_layout(self, n: int | None = None) -> dict:
        """The layouts vrpms_set_instance chose and whether the branch-free
        split takes tours of n customers (default N - 1): the fields of
        vrpms_instance_layout by name, flags as bool, pref_lim as uint32."""
        out = (ctypes.c_int32 * len(self.LAYOUT_FIELDS))()
        check(self.lib.vrpms_instance_layout(self._ctx, self.N - 1 if n is None else int(n), out,
                                             len(out)))
        d = dict(zip(self.LAYOUT_FIELDS, (int(x) for x in out)))
        d["pref_lim"] &= 0xFFFFFFFF
        for k in ("use16", "uniform_cap", "symmetric", "sym_all", "flex", "fast", "carry",
                  "hour_minor"):
            d[k] = bool(d[k])
        return d

    def decode(self, perm, n: int | None = None):
        """Vehicle of each tour position and per-vehicle durations (host lists)."""
        torch = _torch()
        perm = perm.reshape(-1).contiguous()
        n = perm.numel() if n is None else int(n)
        veh = torch.empty(max(n, 1), dtype=torch.int32, device=self.dev)
        dur = torch.empty(self.K, dtype=torch.int32, device=self.dev)
        check(self.lib.vrpms_decode(self._ctx, perm.data_ptr(), perm_dtype_bytes(perm), n,
                                    veh.data_ptr(), dur.data_ptr(), self.stream()))
        return veh[:n].cpu().tolist(), dur.cpu().tolist()

    def argmin(self, keys):
        """(min key, first index) over a key tensor, reduced on the device."""
        torch = _torch()
        out = torch.empty(2, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_argmin(self._ctx, keys.data_ptr(), keys.numel(), out.data_ptr(),
                                    self.stream()))
        k, i = out.cpu().tolist()
        return k & ((1 << 64) - 1), i


    # -- search kernels (state lives in caller-owned device tensors) ----------
    def sa_run(self, cur, cur_key, best, best_key, steps: int, inv_t0: float, inv_alpha: float,
               seed: int, step0: int, window: int = 0, window_types: int = 0, moves: int = 64):
        """Advance every chain (rows of the int16 [chains][n] tensor ``cur``);
        window > 0 samples A11 windowed moves of the A12 types
        ``window_types`` (bit t for move type t, 0 = all); ``moves`` per step
        (64 W: W wavefronts per chain)."""
        chains, n = cur.shape
        p = _lib.SaParams(chains, int(steps), float(inv_t0), float(inv_alpha),
                          int(seed) & (2**64 - 1), int(step0), int(window), int(window_types),
                          int(moves))
        check(self.lib.vrpms_sa_run(self._ctx, ctypes.byref(p), cur.data_ptr(),
                                    cur_key.data_ptr(), best.data_ptr(), best_key.data_ptr(), n,
                                    self.stream()))

    def ga_generation(self, pop, keys, generations: int, pmut: float, seed: int, gen0: int):
        """pop int16 [islands][P][n], keys int64 [islands][P] (must score pop)."""
        islands, P, n = pop.shape
        pm = min(int(round(float(pmut) * 2**32)), 2**32 - 1)
        p = _lib.GaParams(islands, P, int(generations), pm, int(seed) & (2**64 - 1), int(gen0))
        check(self.lib.vrpms_ga_generation(self._ctx, ctypes.byref(p), pop.data_ptr(),
                                           keys.data_ptr(), n, self.stream()))

    def aco_init(self, colonies: int, tau0: int):
        torch = _torch()
        tau = torch.empty((colonies, self.N, self.N), dtype=torch.int32, device=self.dev)
        eta = torch.empty((self.N, self.N), dtype=torch.int32, device=self.dev)
        check(self.lib.vrpms_aco_init(self._ctx, colonies, int(tau0), tau.data_ptr(),
                                      eta.data_ptr(), self.stream()))
        return tau, eta

    def aco_iteration(self, tau, eta, ants: int, seed: int, it: int, evap_shift: int = 3,
                      tau_min: int = 1 << 10, tau_max: int = 1 << 30, best_tours=None,
                      best_keys=None, bsf_period: int = 0):
        """One ACO iteration -> (tours, keys, iteration-best (key, ant) per
        colony); `best_tours`/`best_keys` (per colony) are updated in place
        on the device when given; with `bsf_period` > 0 the best-so-far
        deposits on every bsf_period-th iteration."""
        torch = _torch()
        colonies = tau.shape[0]
        n = self.N - 1
        tours = torch.empty((colonies, ants, n), dtype=torch.int16, device=self.dev)
        keys = torch.empty((colonies, ants), dtype=torch.int64, device=self.dev)
        ib = torch.empty((colonies, 2), dtype=torch.int64, device=self.dev)
        p = _lib.AcoParams(colonies, ants, evap_shift, tau_min, tau_max,
                           int(seed) & (2**64 - 1), int(it), int(bsf_period))
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        check(self.lib.vrpms_aco_iteration(self._ctx, ctypes.byref(p), tau.data_ptr(),
                                           eta.data_ptr(), tours.data_ptr(), keys.data_ptr(),
                                           ib.data_ptr(), ptr(best_tours), ptr(best_keys), n,
                                           self.stream()))
        return tours, keys, ib

    def bf_run(self, n: int, rank_begin: int, rank_end: int):
        """(min key, smallest lexicographic rank) over ranks [begin, end)."""
        torch = _torch()
        out = torch.empty(2, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_bf_run(self._ctx, int(n), int(rank_begin), int(rank_end),
                                    out.data_ptr(), self.stream()))
        k, r = out.cpu().tolist()
        return k & (2**64 - 1), r & (2**64 - 1)

    def tsp_dp(self, n: int):
        """Held-Karp optimum over customers 1..n of the loaded static TSP
        instance -> (key, lexicographically smallest optimal tour).  The
        table (vrpms_tsp_dp_workspace: 2 GiB at n = 24) is a torch tensor, so
        it returns to torch's allocator cache after the call."""
        torch = _torch()
        nbytes = ctypes.c_uint64()
        check(self.lib.vrpms_tsp_dp_workspace(int(n), ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)
        tour = torch.empty(int(n), dtype=torch.int16, device=self.dev)
        key = torch.empty(1, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_tsp_dp_run(self._ctx, int(n), work.data_ptr(), nbytes.value,
                                        tour.data_ptr(), key.data_ptr(), self.stream()))
        k = key.cpu().item()     # synchronises: the table may be released after it
        return k & (2**64 - 1), [int(c) for c in tour.cpu().tolist()]

    def vrp_sp(self, n: int):
        """Set-partitioning optimum (spec A15) over customers 1..n of the
        loaded static CVRP instance, its vehicles and objective -> (key,
        tour of n + K tokens: route 0, separator, ..., route K-1, separator,
        then the unserved customers).  The workspace
        (vrpms_vrp_sp_workspace) is a torch tensor, so it returns to torch's
        allocator cache after the call."""
        torch = _torch()
        nbytes = ctypes.c_uint64()
        check(self.lib.vrpms_vrp_sp_workspace(int(n), int(self.K), ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)
        tour = torch.empty(int(n) + self.K, dtype=torch.int16, device=self.dev)
        key = torch.empty(1, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_vrp_sp_run(self._ctx, int(n), work.data_ptr(), nbytes.value,
                                        tour.data_ptr(), key.data_ptr(), self.stream()))
        k = key.cpu().item()     # synchronises: the workspace may be released after it
        return k & (2**64 - 1), [int(c) for c in tour.cpu().tolist()]

    def tsp_tdp(self, n: int, horizon: int):
        """Time-expanded subset DP (spec A16) over customers 1..n of the
        loaded TSP instance (H = 1 or 24) -> (key, the optimal tour whose
        reversed sequence is lexicographically smallest), the optimum among
        tours of at most `horizon` minutes; (2**64 - 1, zeros) if there is
        none.  The table (vrpms_tsp_tdp_workspace) is a torch tensor, so it
        returns to torch's allocator cache after the call."""
        torch = _torch()
        nbytes = ctypes.c_uint64()
        start = self.start_times[0] if self.start_times else 0
        check(self.lib.vrpms_tsp_tdp_workspace(int(n), int(start), int(horizon),
                                               ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)
        tour = torch.empty(int(n), dtype=torch.int16, device=self.dev)
        key = torch.empty(1, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_tsp_tdp_run(self._ctx, int(n), int(horizon), work.data_ptr(),
                                         nbytes.value, tour.data_ptr(), key.data_ptr(),
                                         self.stream()))
        k = key.cpu().item()     # synchronises: the table may be released after it
        return k & (2**64 - 1), [int(c) for c in tour.cpu().tolist()]

    def vrp_tdsp(self, n: int, horizon: int):
        """Time-expanded partition DP (spec A17) over customers 1..n of the
        loaded CVRP instance (H = 1 or 24), its vehicles, capacities, start
        times and objective -> (key, tour of n + K tokens in vrp_sp's format,
        every route the tie-ruled optimal tour of its customers from its
        vehicle's start time): the optimum among solutions whose every route
        takes at most `horizon` minutes, so the optimum outright when
        `horizon` is at least its primary; a smaller `horizon` may leave more
        customers unvisited, and the caller owns that promise.  The call
        synchronises the stream once on the way (vrpms_vrp_tdsp_run).  The
        workspace (vrpms_vrp_tdsp_workspace) is a torch tensor freed before
        the return."""
        torch = _torch()
        nbytes = ctypes.c_uint64()
        starts = self.start_times or [0]
        check(self.lib.vrpms_vrp_tdsp_workspace(int(n), int(self.K), len(set(starts)),
                                                int(max(starts)), int(horizon),
                                                ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)
        tour = torch.empty(int(n) + self.K, dtype=torch.int16, device=self.dev)
        key = torch.empty(1, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_vrp_tdsp_run(self._ctx, int(n), int(horizon), work.data_ptr(),
                                          nbytes.value, tour.data_ptr(), key.data_ptr(),
                                          self.stream()))
        k = key.cpu().item()     # synchronises: the workspace may be released after it
        del work
        return k & (2**64 - 1), [int(c) for c in tour.cpu().tolist()]

    def tsp_batch_sa(self, mats, steps: int, inv_t0: float, inv_alpha: float, seed: int):
        """One workgroup per request: mats int32 [R][N][N] on the device ->
        (best tours int16 [R][N-1], best keys int64 [R])."""
        torch = _torch()
        R, N, _ = mats.shape
        tours = torch.empty((R, max(N - 1, 1)), dtype=torch.int16, device=self.dev)
        keys = torch.empty(R, dtype=torch.int64, device=self.dev)
        p = _lib.SaParams(4 * R, int(steps), float(inv_t0), float(inv_alpha),
                          int(seed) & (2**64 - 1), 0, 0)
        check(self.lib.vrpms_tsp_batch_sa(self._ctx, mats.data_ptr(), R, N, ctypes.byref(p),
                                          tours.data_ptr(), keys.data_ptr(), self.stream()))
        return tours, keys

    def _batch_mats(self, torch, mats, rank: int):
        """The batched wrappers' `mats` check: contiguous int32 [R][N][N]
        (rank 3) or [R][H][N][N] (rank 4, [R][N][N] taken as H = 1) here."""
        if rank == 4 and mats.dim() == 3:
            mats = mats.unsqueeze(1)
        if mats.device != self.dev or mats.dim() != rank or mats.shape[-2] != mats.shape[-1] or \
                mats.dtype != torch.int32 or not mats.is_contiguous():
            raise ValueError(f"mats must be a contiguous int32 [R]{'[H]' * (rank - 3)}[N][N] "
                             f"tensor on {self.dev}")
        return mats

    def _batch_rows(self, torch, demand, caps, R: int, N: int):
        """demand is a contiguous int32 [R][N] tensor here, caps an [R][K] one."""
        for name, t, cols in (("demand", demand, N), ("caps", caps, None)):
            if t.device != self.dev or t.dim() != 2 or t.shape[0] != R or t.dtype != torch.int32 or \
                    not t.is_contiguous() or (cols is not None and t.shape[1] != cols):
                raise ValueError(f"{name} must be a contiguous int32 [R][{'N' if cols else 'K'}] "
                                 f"tensor on {self.dev}")

    def _vrp_batch_args(self, mats, demand, caps, starts, wide):
        """The batched heuristics' VRP arguments, checked: mats of rank 4,
        demand [R][N], caps and starts [R][K] -> (mats, R, H, N, K, wide), a
        `wide` of None answered by the device (_wide)."""
        torch = _torch()
        mats = self._batch_mats(torch, mats, 4)
        R, H, N, _ = mats.shape
        self._batch_rows(torch, demand, caps, R, N)
        if starts.device != self.dev or starts.shape != caps.shape or starts.dtype != torch.int32 \
                or not starts.is_contiguous():
            raise ValueError(f"starts must be a contiguous int32 [R][K] tensor on {self.dev}")
        return mats, R, H, N, caps.shape[1], self._wide(mats, wide)

    def _tsp_batch_args(self, mats, starts, wide):
        """The TSP counterpart: mats of rank 4 and starts [R] -> (mats, R, H, N,
        wide)."""
        torch = _torch()
        mats = self._batch_mats(torch, mats, 4)
        R, H, N, _ = mats.shape
        if starts.device != self.dev or starts.shape != (R,) or starts.dtype != torch.int32 \
                or not starts.is_contiguous():
            raise ValueError(f"starts must be a contiguous int32 [R] tensor on {self.dev}")
        return mats, R, H, N, self._wide(mats, wide)

    @staticmethod
    def _wide(mats, wide):
        """`wide` as given, or for None whether the batch's largest entry is
        above 65535: a question to the device, which synchronises."""
        return (bool(mats.shape[0]) and int(mats.max().item()) > 65535) if wide is None else wide

    def _batch_out(self, R: int, ntok: int, K: int | None = None, info: bool = False) -> tuple:
        """The batched heuristics' output tensors, in the entry points' order:
        tours int16 [R][ntok], keys int64 [R], durs int32 [R][K] ([R] without
        a K: a TSP's), with a K veh int8 [R][ntok], with `info` info int32
        [R][2]."""
        torch = _torch()
        shapes = [((R, max(ntok, 1)), torch.int16), (R, torch.int64),
                  (R if K is None else (R, max(K, 1)), torch.int32)]
        if K is not None:
            shapes.append(((R, max(ntok, 1)), torch.int8))
        if info:
            shapes.append(((R, 2), torch.int32))
        return tuple(torch.empty(shape, dtype=dtype, device=self.dev) for shape, dtype in shapes)

    def _spread_work(self, size, R: int, shape, groups: int, nstarts: int):
        """The workspace of a spread launch of R requests of `shape` at
        min(groups, nstarts) workgroups each, `size` its size function ->
        (groups as an int, the workspace, its bytes); groups outside 1..65535
        is left to the entry point to refuse."""
        G = int(groups)
        nbytes = size(R, *shape, max(1, min(G, int(nstarts)))) if R and 1 <= G <= 65535 else 0
        return G, _torch().empty(max(nbytes // 8, 1), dtype=_torch().int64, device=self.dev), nbytes

    def _host_minutes(self, torch, starts, shape, horizons, R: int, explicit: bool):
        """starts (of `shape`) and horizons ([R]) as int64 host arrays for the
        caller to check and upload, or None when both are int32 tensors of
        those shapes here and the launch's widths are `explicit`: uploaded and
        checked by the caller, passed through as they are."""
        if explicit and all([isinstance(t, torch.Tensor) and t.device == self.dev and
                             t.dtype == torch.int32 and t.shape == sh and t.is_contiguous()
                             for t, sh in ((starts, shape), (horizons, (R,)))]):
            return None
        return [(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.int64)
                for t in (starts, horizons)]

    def tsp_batch_dp(self, mats):
        """Exact optimum of every request in one launch (spec A18, at most 12
        customers): mats int32 [R][N][N] on the device -> (tours int16
        [R][N-1], keys int64 [R]), per request what tsp_dp returns for that
        matrix.  N * max(mats) < 2^31 (A9) is the caller's promise: whoever
        builds `mats` from host data checks it before uploading.
        Asynchronous on the current stream."""
        torch = _torch()
        R, N, _ = self._batch_mats(torch, mats, 3).shape
        tours = torch.empty((R, max(N - 1, 1)), dtype=torch.int16, device=self.dev)
        keys = torch.empty(R, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_tsp_batch_dp(self._ctx, mats.data_ptr(), R, N, tours.data_ptr(),
                                          keys.data_ptr(), self.stream()))
        return tours, keys

    def vrp_batch_sp(self, mats, demand, caps, objective: int = OBJ_SUM, team: int = 0):
        """Exact VRP optimum of every request in one launch (spec A19, at most
        12 customers, all requests of one N, K and objective): mats int32
        [R][N][N], demand int32 [R][N] (entry 0 ignored) and caps int32 [R][K]
        on the device -> (tours int16 [R][N-1+K], keys int64 [R], durs int32
        [R][K]), per request the tour and key vrp_sp returns for that instance
        and its K route durations, unclamped.  `team`: threads per request, 0 =
        auto, or 16, 32, 64, 128, 256 (the answers do not depend on it).
        (N + K + 1) * max(mats) < 2^31 (A9) and non-negative demands and
        capacities are the caller's promise: whoever builds the buffers from
        host data checks them before uploading.  Asynchronous on the current
        stream."""
        torch = _torch()
        R, N, _ = self._batch_mats(torch, mats, 3).shape
        self._batch_rows(torch, demand, caps, R, N)
        K = caps.shape[1]
        tours = torch.empty((R, max(N - 1 + K, 1)), dtype=torch.int16, device=self.dev)
        keys = torch.empty(R, dtype=torch.int64, device=self.dev)
        durs = torch.empty((R, max(K, 1)), dtype=torch.int32, device=self.dev)
        check(self.lib.vrpms_vrp_batch_sp(self._ctx, mats.data_ptr(), demand.data_ptr(),
                                          caps.data_ptr(), R, N, K, int(objective), int(team),
                                          tours.data_ptr(), keys.data_ptr(), durs.data_ptr(),
                                          self.stream()))
        return tours, keys, durs

    def tsp_batch_tdp(self, mats, starts, horizons, W: int | None = None, team: int = 0):
        """Exact time-dependent optimum of every request in one launch (spec
        A20, at most 11 customers, all requests of one N and H): mats int32
        [R][H][N][N] (H = 1 or 24; [R][N][N] is taken as H = 1), starts and
        horizons [R] (host sequences, numpy arrays or tensors; minutes, >= 0;
        int32 tensors on the device together with an explicit `W` are passed
        through as they are) -> (tours int16 [R][N-1], keys int64 [R]), per request what tsp_tdp
        returns for that matrix, start and horizon: all-ones key and a zero
        tour where no tour fits the horizon.  `W`: the launch's row width in
        hour words, default the largest tdp_words(start, horizon) of the
        batch, computed on the host; a smaller one can prune an answer (the
        effective horizon is min(horizon, 60 W - 1 - start % 60)).  `team`:
        threads per request, 0 = auto, or 16, 32, 64, 128, 256 (the answers do
        not depend on it).  Non-negative durations are the caller's promise.
        Asynchronous on the current stream."""
        torch = _torch()
        mats = self._batch_mats(torch, mats, 4)
        R, H, N, _ = mats.shape
        host = self._host_minutes(torch, starts, (R,), horizons, R, W is not None)
        if host is None:
            d_st, d_hz = starts, horizons
        else:
            st, hz = host[0].reshape(-1), host[1].reshape(-1)
            for name, a in (("starts", st), ("horizons", hz)):
                if a.shape[0] != R:
                    raise ValueError(f"{name} must have one entry per request ({R})")
                if R and (a.min() < 0 or a.max() >= 2**31):
                    raise ValueError(f"{name} must be non-negative int32 minutes")
            if R and int((st + hz).max()) >= 2**31:
                raise ValueError("start + horizon must stay below 2^31")
            if W is None:
                W = int(((st % 60 + hz) // 60 + 1).max()) if R else 1
            d_st = torch.from_numpy(st.astype(np.int32)).to(self.dev)
            d_hz = torch.from_numpy(hz.astype(np.int32)).to(self.dev)
        tours = torch.empty((R, max(N - 1, 1)), dtype=torch.int16, device=self.dev)
        keys = torch.empty(R, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_tsp_batch_tdp(self._ctx, mats.data_ptr(), d_st.data_ptr(),
                                           d_hz.data_ptr(), R, N, H, int(W), int(team),
                                           tours.data_ptr(), keys.data_ptr(), self.stream()))
        return tours, keys

    def vrp_batch_tdsp(self, mats, demand, caps, starts, horizons, objective: int = OBJ_SUM,
                       G: int | None = None, W: int | None = None, team: int = 0):
        """Exact time-dependent VRP optimum of every request in one launch
        (spec A21, at most 11 customers, all requests of one N, K, H and
        objective): mats int32 [R][H][N][N] (H = 1 or 24; [R][N][N] is taken
        as H = 1), demand int32 [R][N] (entry 0 ignored) and caps int32 [R][K]
        on the device, starts [R][K] and horizons [R] (host sequences, numpy
        arrays or tensors; minutes, >= 0; int32 tensors on the device
        together with explicit `G` and `W` are passed through as they are)
        -> (tours int16 [R][N-1+K], keys int64 [R], durs int32 [R][K]), per
        request the tour and key vrp_tdsp returns for that instance and
        horizon and its K route durations, unclamped.  `G`: the launch's
        limit on one request's distinct start times, `W`: its row width in
        hour words; both default to the batch's largest need, computed on
        the host.  A request with more than G distinct starts gets an
        all-ones key, a zero tour and durations of -1; a smaller W can prune
        an answer (for a start s the effective horizon is min(horizon, 60 W -
        1 - s % 60)).  `team`: threads per request, 0 = auto, or 16, 32, 64,
        128, 256 (the answers do not depend on it).  The A9 guard and
        non-negative durations, demands and capacities are the caller's
        promise.  Asynchronous on the current stream."""
        torch = _torch()
        mats = self._batch_mats(torch, mats, 4)
        R, H, N, _ = mats.shape
        self._batch_rows(torch, demand, caps, R, N)
        K = caps.shape[1]
        host = self._host_minutes(torch, starts, (R, K), horizons, R,
                                  W is not None and G is not None)
        if host is None:
            d_st, d_hz = starts, horizons
        else:
            st, hz = host[0], host[1].reshape(-1)
            if st.size != R * K:
                raise ValueError(f"starts must have one row of {K} start times per request ({R})")
            st = st.reshape(R, K)
            if hz.shape[0] != R:
                raise ValueError(f"horizons must have one entry per request ({R})")
            if R and K and (min(st.min(), hz.min()) < 0 or max(st.max(), hz.max()) >= 2**31):
                raise ValueError("starts and horizons must be non-negative int32 minutes")
            if R and K and int((st.max(axis=1) + hz).max()) >= 2**31:
                raise ValueError("start + horizon must stay below 2^31")
            if W is None:
                W = int(((st % 60 + hz[:, None]) // 60 + 1).max()) if R and K else 1
            if G is None:
                G = max((len(set(row)) for row in st.tolist()), default=1) if K else 1
            d_st = torch.from_numpy(st.astype(np.int32)).to(self.dev)
            d_hz = torch.from_numpy(hz.astype(np.int32)).to(self.dev)
        tours = torch.empty((R, max(N - 1 + K, 1)), dtype=torch.int16, device=self.dev)
        keys = torch.empty(R, dtype=torch.int64, device=self.dev)
        durs = torch.empty((R, max(K, 1)), dtype=torch.int32, device=self.dev)
        check(self.lib.vrpms_vrp_batch_tdsp(self._ctx, mats.data_ptr(), demand.data_ptr(),
                                            caps.data_ptr(), d_st.data_ptr(), d_hz.data_ptr(), R, N,
                                            K, int(G), H, int(W), int(objective), int(team),
                                            tours.data_ptr(), keys.data_ptr(), durs.data_ptr(),
                                            self.stream()))
        return tours, keys, durs

    def vrp_batch_sa(self, mats, demand, caps, starts, inv_t0, objective: int, steps: int,
                     inv_alpha: float, seed: int, wide=None):
        """Four annealing chains per request, one workgroup per request, one
        launch for all (spec A22; all requests of one N, K, H and objective):
        mats int32 [R][H][N][N] (H = 1 or 24; [R][N][N] is taken as H = 1),
        demand int32 [R][N] (entry 0 ignored), caps and starts int32 [R][K]
        and inv_t0 float32 [R] on the device -> (tours int16 [R][ntok], keys
        int64 [R], durs int32 [R][K], veh int8 [R][ntok]) with ntok = N - 1 +
        K - 1: per request the best tour of its four chains, its A8 key, its K
        route durations (unclamped, 0 for an empty route) and the vehicle of
        every token (-1 unvisited, -2 separator).  A request's row depends on
        the request, `steps`, its inv_t0, `inv_alpha`, `seed` and `objective`
        alone, not on the batch.  `wide`: False stages the matrices as uint16
        (a request with an entry above 65535 then gets an all-ones key, a zero
        tour, zero durations and veh = -1), True as int32; whoever builds
        `mats` from host data knows which, so None -- the default -- asks the
        device for the batch's largest entry, which synchronises.  The A9
        guard and non-negative demands and capacities are the caller's
        promise.  Asynchronous on the current stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        if inv_t0.device != self.dev or inv_t0.shape != (R,) or \
                inv_t0.dtype != _torch().float32 or not inv_t0.is_contiguous():
            raise ValueError(f"inv_t0 must be a contiguous float32 [R] tensor on {self.dev}")
        out = self._batch_out(R, N - 1 + K - 1, K)
        check(self.lib.vrpms_vrp_batch_sa(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(),
            inv_t0.data_ptr(), R, N, K, H, int(objective), int(bool(wide)), int(steps),
            float(inv_alpha), _u64(seed), *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_ga(self, mats, demand, caps, starts, objective: int, pop: int, gens: int,
                     pmut: float, seed: int, wide=None):
        """A genetic algorithm per request, one workgroup per request, one
        launch for all (spec A23; all requests of one N, K, H and objective):
        mats int32 [R][H][N][N] (H = 1 or 24; [R][N][N] is taken as H = 1),
        demand int32 [R][N] (entry 0 ignored), caps and starts int32 [R][K] on
        the device -> (tours int16 [R][n], keys int64 [R], durs int32 [R][K],
        veh int8 [R][n]) with n = N - 1: per request the member of the least
        (key, index) after `gens` generations of a population of `pop`
        (2..256) separator-free tours, its A8 key, its K route durations
        (unclamped, 0 for an empty route) and the vehicle of every gene (-1
        unvisited).  `pmut` is the mutation probability, converted as
        ga_generation does: min(round(pmut * 2^32), 2^32 - 1).  A request's
        row depends on the request, `pop`, `gens`, `pmut`, `seed` and
        `objective` alone, not on the batch.  `wide`: False stages the
        matrices as uint16 (a request with an entry above 65535 then gets an
        all-ones key, a zero tour, zero durations and veh = -1), True as
        int32; None -- the default -- asks the device for the batch's largest
        entry, which synchronises.  The A9 guard and non-negative demands and
        capacities are the caller's promise.  Asynchronous on the current
        stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        pm = min(int(round(float(pmut) * 2**32)), 2**32 - 1)
        out = self._batch_out(R, N - 1, K)
        check(self.lib.vrpms_vrp_batch_ga(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(pop), int(gens), pm, _u64(seed),
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_aco(self, mats, demand, caps, starts, objective: int, ants: int, iters: int,
                      seed: int, wide=None, tau0: int = 1 << 24, tau_min: int = 1 << 12,
                      tau_max: int = 1 << 30, evap_shift: int = 3, bsf_period: int = 5):
        """An ant colony per request, one workgroup per request, one launch
        for all (spec A24; all requests of one N, K, H and objective): mats
        int32 [R][H][N][N] (H = 1 or 24; [R][N][N] is taken as H = 1), demand
        int32 [R][N] (entry 0 ignored), caps and starts int32 [R][K] on the
        device -> (tours int16 [R][n], keys int64 [R], durs int32 [R][K], veh
        int8 [R][n]) with n = N - 1: per request the best-so-far tour of one
        colony of `ants` (1..256) ants after `iters` (>= 1) iterations, its A8
        key, its K route durations (unclamped, 0 for an empty route) and the
        vehicle of every customer of the tour (-1 unvisited).  The pheromone
        parameters default to ACORunner's, and with them the row is the
        best-so-far of ACORunner(ctx, n, colonies=1, ants=ants, seed=seed)
        stepped `iters` times on the same instance.  A request's row depends
        on the request, `ants`, `iters`, the pheromone parameters, `seed` and
        `objective` alone, not on the batch.  `wide`: False stages the
        matrices as uint16 (a request with an entry above 65535 then gets an
        all-ones key, a zero tour, zero durations and veh = -1), True as
        int32; None -- the default -- asks the device for the batch's largest
        entry, which synchronises.  The A9 guard and non-negative demands and
        capacities are the caller's promise.  Asynchronous on the current
        stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        for name, v in (("tau0", tau0), ("tau_min", tau_min), ("tau_max", tau_max)):
            if not 0 <= int(v) < 2**32:
                raise ValueError(f"{name} must be a uint32")
        out = self._batch_out(R, N - 1, K)
        check(self.lib.vrpms_vrp_batch_aco(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(ants), int(iters), int(tau0), int(tau_min),
            int(tau_max), int(evap_shift), int(bsf_period), _u64(seed),
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_ls(self, mats, demand, caps, starts, objective: int, nstarts: int, rounds: int,
                     seed: int, wide=None):
        """A multi-start local search per request, one workgroup per request,
        one launch for all (spec A25; all requests of one N, K, H and
        objective): mats int32 [R][H][N][N] (H = 1 or 24; [R][N][N] is taken as
        H = 1), demand int32 [R][N] (entry 0 ignored), caps and starts int32
        [R][K] on the device -> (tours int16 [R][n], keys int64 [R], durs
        int32 [R][K], veh int8 [R][n], info int32 [R][2]) with n = N - 1: per
        request the least (key, start) end tour of `nstarts` (1..65535)
        steepest descents over swap, 2-opt and relocate from vrp_batch_ga's
        random members 0..nstarts-1, each stopped at a local optimum or after
        `rounds` (>= 0) applied moves; its A8 key, its K route durations
        (unclamped, 0 for an empty route), the vehicle of every gene (-1
        unvisited), and info = (the winning start, the number of descents the
        round cap stopped unproven).  A request's row depends on the request,
        `nstarts`, `rounds`, `seed` and `objective` alone, not on the batch.
        `wide`: False stages the matrices as uint16 (a request with an entry
        above 65535 then gets an all-ones key, a zero tour, zero durations,
        veh = -1 and info = (-1, 0)), True as int32; None -- the default --
        asks the device for the batch's largest entry, which synchronises.
        The A9 guard and non-negative demands and capacities are the caller's
        promise.  Asynchronous on the current stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        out = self._batch_out(R, N - 1, K, info=True)
        check(self.lib.vrpms_vrp_batch_ls(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(nstarts), int(rounds), _u64(seed),
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def tsp_batch_lso(self, mats, starts, nstarts: int, rounds: int, moves: int, seed: int,
                      wide=None):
        """A multi-start local search with Or-opt moves and delta pricing per
        TSP request, one workgroup per request, one launch for all (spec A27;
        all requests of one N and H): mats int32 [R][H][N][N] (H = 1 or 24;
        [R][N][N] is taken as H = 1) and starts int32 [R] (the start times,
        minutes) on the device -> (tours int16 [R][n], keys int64 [R], durs
        int32 [R], info int32 [R][2]) with n = N - 1: per request the least
        (key, start) end tour of `nstarts` (1..65535) steepest descents from
        vrp_batch_ls's random starts 0..nstarts-1 over the move types `moves`
        enables (1..31; bit 0 swap, 1 2-opt, 2 relocate, 3 and 4 Or-opt of two
        and three customers), each stopped at a local optimum or after `rounds`
        (>= 0) applied moves; its key (spec.tsp_key), its unclamped duration,
        and info = (the winning start, the number of descents the round cap
        stopped unproven).  A request's row depends on the request, `nstarts`,
        `rounds`, `moves` and `seed` alone, not on the batch; with moves = 7
        the tour and info are vrp_batch_ls's at K = 1 and zero demands.
        `wide`: False stages the matrices as uint16 (a request with an entry
        above 65535 then gets an all-ones key, a zero tour, duration 0 and
        info = (-1, 0)), True as int32; None -- the default -- asks the device
        for the batch's largest entry, which synchronises.  The A9 guard is
        the caller's promise.  Asynchronous on the current stream."""
        mats, R, H, N, wide = self._tsp_batch_args(mats, starts, wide)
        out = self._batch_out(R, N - 1, info=True)
        check(self.lib.vrpms_tsp_batch_lso(
            self._ctx, mats.data_ptr(), starts.data_ptr(), R, N, H, int(bool(wide)), int(nstarts),
            int(rounds), int(moves), _u64(seed), *(t.data_ptr() for t in out), self.stream()))
        return out

    def tsp_batch_lso_spread(self, mats, starts, nstarts: int, rounds: int, moves: int, seed: int,
                             groups: int, wide=None):
        """tsp_batch_lso by another mapping: the same
        arguments and the identical four tensors, but a request's `nstarts`
        starts are spread over min(`groups`, nstarts) workgroups (`groups` in
        1..65535) whose 256 threads each price one round of one tour together,
        and a second launch selects the least (key, start) per request.  For
        few requests that occupies R * groups workgroups instead of R.  The
        workspace (tsp_batch_lso_spread_work) is allocated here, from torch's
        caching allocator, which keeps it alive for the stream's queued work.
        Asynchronous on the current stream."""
        mats, R, H, N, wide = self._tsp_batch_args(mats, starts, wide)
        G, work, work_bytes = self._spread_work(tsp_batch_lso_spread_work, R, (N,), groups, nstarts)
        out = self._batch_out(R, N - 1, info=True)
        check(self.lib.vrpms_tsp_batch_lso_spread(
            self._ctx, mats.data_ptr(), starts.data_ptr(), R, N, H, int(bool(wide)), int(nstarts),
            int(rounds), int(moves), _u64(seed), G, work.data_ptr(), work_bytes,
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_lsr(self, mats, demand, caps, starts, objective: int, nstarts: int, rounds: int,
                      seed: int, wide=None):
        """A multi-start local search over separator tours per request, one
        workgroup per request, one launch for all (spec A26; all requests of
        one N, K, H and objective): vrp_batch_ls's arguments -> (tours int16
        [R][L], keys int64 [R], durs int32 [R][K], veh int8 [R][L], info int32
        [R][2]) with L = N - 1 + K - 1 tokens, 0 a route separator: per
        request the least (key, start) end tour of `nstarts` (1..65535)
        steepest descents over swap, 2-opt and relocate on all L positions,
        start s being vrp_batch_ls's start s packed first-fit into the K
        routes as vrp_batch_sa packs its chains', each stopped at a local
        optimum or after `rounds` (>= 0) applied moves; its A8 key, its K route
        durations (unclamped, 0 for an empty route), the vehicle of every token
        (-1 unvisited, -2 a separator), and info = (the winning start, the
        number of descents the round cap stopped unproven).  A request's row
        depends on the request, `nstarts`, `rounds`, `seed` and `objective`
        alone, not on the batch.  `wide`: False stages the matrices as uint16
        (a request with an entry above 65535 then gets an all-ones key, a zero
        tour, zero durations, veh = -1 and info = (-1, 0)), True as int32;
        None -- the default -- asks the device for the batch's largest entry,
        which synchronises.  The A9 guard and non-negative demands and
        capacities are the caller's promise.  Asynchronous on the current
        stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        out = self._batch_out(R, N - 1 + K - 1, K, info=True)
        check(self.lib.vrpms_vrp_batch_lsr(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(nstarts), int(rounds), _u64(seed),
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_lsf(self, mats, demand, caps, starts, objective: int, nstarts: int, rounds: int,
                      seed: int, wide=None):
        """vrp_batch_lsr on the plain separator tours of a static matrix, with
        delta pricing (spec A28): the same arguments (H = 1
        only) and the same five tensors.  A tour is plain when the customers
        between separator g - 1 and separator g weigh at most caps[g]; a move
        onto a tour that is not plain is no candidate, and a start that is not
        plain ends where it starts and is never capped.  With every capacity
        at least the total demand the tensors are vrp_batch_lsr's bit for bit.
        An hour-indexed batch is refused: it keeps vrp_batch_lsr.
        Asynchronous on the current stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        out = self._batch_out(R, N - 1 + K - 1, K, info=True)
        check(self.lib.vrpms_vrp_batch_lsf(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(nstarts), int(rounds), _u64(seed),
            *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_lsr_spread(self, mats, demand, caps, starts, objective: int, nstarts: int,
                             rounds: int, seed: int, groups: int, wide=None):
        """vrp_batch_lsr by another mapping: the same
        arguments and the identical five tensors, but a request's `nstarts`
        starts are spread over min(`groups`, nstarts) workgroups (`groups` in
        1..65535) whose 256 threads each price one round of one tour together,
        and a second launch selects the least (key, start) per request.  For
        few requests that occupies R * groups workgroups instead of R.  The
        workspace (vrp_batch_lsr_spread_work) is allocated here, from torch's
        caching allocator, which keeps it alive for the stream's queued work.
        Asynchronous on the current stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        G, work, work_bytes = self._spread_work(vrp_batch_lsr_spread_work, R, (N, K), groups,
                                                nstarts)
        out = self._batch_out(R, N - 1 + K - 1, K, info=True)
        check(self.lib.vrpms_vrp_batch_lsr_spread(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(nstarts), int(rounds), _u64(seed), G,
            work.data_ptr(), work_bytes, *(t.data_ptr() for t in out), self.stream()))
        return out

    def vrp_batch_lsf_spread(self, mats, demand, caps, starts, objective: int, nstarts: int,
                             rounds: int, seed: int, groups: int, wide=None):
        """vrp_batch_lsf by vrp_batch_lsr_spread's mapping:
        the same arguments (H = 1 only) and the identical five tensors, but a
        request's `nstarts` starts are spread over min(`groups`, nstarts)
        workgroups (`groups` in 1..65535) whose 256 threads each price one
        round of one plain tour together, and a second launch selects the
        least (key, start) per request.  For few requests that occupies
        R * groups workgroups instead of R.  The workspace
        (vrp_batch_lsf_spread_work) is allocated here, from torch's caching
        allocator, which keeps it alive for the stream's queued work.
        Asynchronous on the current stream."""
        mats, R, H, N, K, wide = self._vrp_batch_args(mats, demand, caps, starts, wide)
        G, work, work_bytes = self._spread_work(vrp_batch_lsf_spread_work, R, (N, K), groups,
                                                nstarts)
        out = self._batch_out(R, N - 1 + K - 1, K, info=True)
        check(self.lib.vrpms_vrp_batch_lsf_spread(
            self._ctx, mats.data_ptr(), demand.data_ptr(), caps.data_ptr(), starts.data_ptr(), R, N,
            K, H, int(objective), int(bool(wide)), int(nstarts), int(rounds), _u64(seed), G,
            work.data_ptr(), work_bytes, *(t.data_ptr() for t in out), self.stream()))
        return out

    def set_batch_dp_team(self, T: int):
        """Threads per request of tsp_batch_dp: 0 = auto (the n -> T table),
        16, 32, 64, 128 or 256 force (A/B; the results do not depend on it)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_BATCH_DP_TEAM, int(T)))

    # -- populations and the island model (pool.hip) ---------------------------
    def random_tours(self, count: int, n: int, seed: int, stream_id: int = 0, ld: int | None = None,
                     dtype=None, n_sep: int = 0):
        """Philox Fisher-Yates permutations of 1..n plus `n_sep` route
        separators (token 0, A10) -- vrpms_random_tours -- as int16 (default)
        or uint8 rows of `ld` elements."""
        torch = _torch()
        dtype = torch.int16 if dtype is None else dtype
        ld = n + n_sep if ld is None else int(ld)
        out = torch.zeros((int(count), ld), dtype=dtype, device=self.dev)
        check(self.lib.vrpms_random_tours(self._ctx, int(count), int(n), int(n_sep), ld,
                                          perm_dtype_bytes(out), int(seed) & (2**64 - 1),
                                          int(stream_id) & 0xFFFFFFFF, out.data_ptr(),
                                          self.stream()))
        return out

    def insert_separators(self, tours, n_sep: int):
        """int16 [count][n] customer tours -> [count][n + n_sep] with A10
        separators at the greedy split's route boundaries (vrpms_insert_separators)."""
        torch = _torch()
        count, n = tours.shape
        out = torch.empty((count, n + int(n_sep)), dtype=torch.int16, device=self.dev)
        check(self.lib.vrpms_insert_separators(self._ctx, tours.contiguous().data_ptr(), count, n,
                                               int(n_sep), out.data_ptr(), self.stream()))
        return out

    def pack_separators(self, tours, n_sep: int):
        """int16 [count][n] customer tours -> [count][n + n_sep]: first-fit
        routes in input order, one separator between consecutive routes
        (vrpms_pack_separators)."""
        torch = _torch()
        count, n = tours.shape
        out = torch.empty((count, n + int(n_sep)), dtype=torch.int16, device=self.dev)
        check(self.lib.vrpms_pack_separators(self._ctx, tours.contiguous().data_ptr(), count, n,
                                             int(n_sep), out.data_ptr(), self.stream()))
        return out

    @staticmethod
    def pool(tours, keys, groups: int = 1):
        """vrpms_pool over an int16 [count][n] (or [g][p][n]) tour tensor and its keys."""
        count = keys.numel()
        n = tours.shape[-1]
        if tours.numel() != count * n or not tours.is_contiguous() or not keys.is_contiguous():
            raise ValueError("pool: tours must be a contiguous [count][n] tensor matching keys")
        return _lib.Pool(tours.data_ptr(), keys.data_ptr(), count, n, int(groups))

    def pool_elites(self, tours, keys, E: int):
        """The E best rows by (key, index) -> (tours [E][n], keys [E])."""
        torch = _torch()
        n = tours.shape[-1]
        t = torch.empty((E, n), dtype=torch.int16, device=self.dev)
        k = torch.empty(E, dtype=torch.int64, device=self.dev)
        p = self.pool(tours, keys)
        check(self.lib.vrpms_pool_elites(self._ctx, ctypes.byref(p), int(E), t.data_ptr(),
                                         k.data_ptr(), self.stream()))
        return t, k

    def pool_inject(self, tours, keys, mode: int, mig_tours, mig_keys, groups: int = 1):
        p = self.pool(tours, keys, groups)
        mt = mig_tours.to(_torch().int16).contiguous()
        mk = mig_keys.contiguous()
        check(self.lib.vrpms_pool_inject(self._ctx, ctypes.byref(p), int(mode), mt.data_ptr(),
                                         mk.data_ptr(), int(mk.numel()), self.stream()))

    def island_msg_bytes(self, E: int, n: int) -> int:
        return int(self.lib.vrpms_island_msg_bytes(int(E), int(n)))

    def island_pack(self, tours, keys, E: int):
        """The E elites as one island message (uint8 device tensor)."""
        torch = _torch()
        n = tours.shape[-1]
        msg = torch.empty(self.island_msg_bytes(E, n), dtype=torch.uint8, device=self.dev)
        p = self.pool(tours, keys)
        check(self.lib.vrpms_island_pack(self._ctx, ctypes.byref(p), int(E), msg.data_ptr(),
                                         self.stream()))
        return msg

    def island_merge(self, msgs, world: int, E: int, n: int):
        """The E best of `world` gathered messages -> (tours [E][n], keys [E])."""
        torch = _torch()
        msgs = msgs.to(self.dev).contiguous()
        t = torch.empty((E, n), dtype=torch.int16, device=self.dev)
        k = torch.empty(E, dtype=torch.int64, device=self.dev)
        check(self.lib.vrpms_island_merge(self._ctx, msgs.data_ptr(), int(world), int(E), int(n),
                                          t.data_ptr(), k.data_ptr(), self.stream()))
        return t, k

    def island_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        check(self.lib.vrpms_island_unique_id(buf))
        return buf.raw

    def island_init(self, unique_id: bytes, rank: int, world: int):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self.lib.vrpms_island_init(self._ctx, buf, int(rank), int(world)))

    def island_world(self) -> int:
        return int(self.lib.vrpms_island_world(self._ctx))

    def set_island_timeout(self, seconds: int):
        """Deadline of vrpms_island_init (VRPMS_OPT_ISLAND_TIMEOUT_S)."""
        check(self.lib.vrpms_set_option(self._ctx, _lib.OPT_ISLAND_TIMEOUT_S, int(seconds)))

    def island_exchange(self, src, dst, mode: int, E: int, groups: int = 1):
        """vrpms_island_exchange: src/dst are (tours, keys) pairs."""
        ps = self.pool(*src)
        pd = self.pool(*dst, groups=groups)
        check(self.lib.vrpms_island_exchange(self._ctx, ctypes.byref(ps), ctypes.byref(pd),
                                             int(mode), int(E), self.stream()))

    def probe_lds_gather(self, slots: int = 101 * 101, iters: int = 4096, blocks: int | None = None,
                         reps: int = 5):
        """Measured random ds_read_b64 gather rate (gathers/s), best of `reps`."""
        torch = _torch()
        blocks = blocks or 2 * 256
        table = torch.randint(0, 2**62, (slots,), dtype=torch.int64, device=self.dev)
        sink = torch.zeros(1, dtype=torch.int64, device=self.dev)
        best = 0.0
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(self.lib.vrpms_probe_lds_gather(self._ctx, table.data_ptr(), slots, iters,
                                                  blocks, sink.data_ptr(), self.stream()))
            e1.record()
            torch.cuda.synchronize(self.dev)
            best = max(best, blocks * 1024 * 4 * iters / (e0.elapsed_time(e1) * 1e-3))
        return best

    def probe_l2_gather(self, slots: int = 24 * 201 * 201, iters: int = 256,
                        blocks: int | None = None, reps: int = 5):
        """Measured random 2-byte global-load gather rate (gathers/s) over an
        L2-resident uint16 table of `slots` entries, best of `reps`."""
        torch = _torch()
        blocks = blocks or 8 * 256 * 4
        table = torch.randint(0, 2**15, (slots,), dtype=torch.int16, device=self.dev)
        sink = torch.zeros(1, dtype=torch.int64, device=self.dev)
        best = 0.0
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(self.lib.vrpms_probe_l2_gather(self._ctx, table.data_ptr(), slots, iters,
                                                 blocks, sink.data_ptr(), self.stream()))
            e1.record()
            torch.cuda.synchronize(self.dev)
            best = max(best, blocks * 256 * 8 * iters / (e0.elapsed_time(e1) * 1e-3))
        return best


def keys_to_u64(keys) -> np.ndarray:
    """int64 tensor of A8 keys -> numpy uint64 (bit-identical view)."""
    return keys.cpu().numpy().view(np.uint64)
