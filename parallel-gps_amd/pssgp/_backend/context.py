"""Context: one GPU, one stream, its scratch and knobs; get_context() keeps one per device."""
import ctypes
import threading

import numpy as np

from .. import _backend as _facade      # `check` is looked up there at every call: tests wrap it to record the routes
from .arrays import _ptr
from .library import COMM_ID_BYTES, PGPS_OK, PgpsError, c_double, c_int, c_long, c_void_p, load_library


class Context:
    """One libpgps context = one GPU + one stream + scratch (+ the RCCL communicator of a sharded series).

    libpgps allows one call in flight per context (include/pgps.h); `lock` (re-entrant) serialises the calls made
    through this object, so Python threads that share a context -- e.g. parallel MCMC chains on the default
    context of `get_context` -- take turns instead of racing on its scratch.  Multi-call sequences that keep state
    in the context (LtiLlStream, the three-phase segment protocol) hold the lock for their whole duration."""

    def __init__(self, device=0):
        self.lock = threading.RLock()
        self.lib = load_library()
        n = c_int(0)
        self.lib.pgps_device_count(ctypes.byref(n))
        if n.value <= 0:
            raise PgpsError(-6, "no HIP device visible: the parallel path needs an MI355X (there is no CPU fallback)")
        self.handle = c_void_p()
        code = self.lib.pgps_create(int(device), ctypes.byref(self.handle))
        if code != PGPS_OK:
            raise PgpsError(code, "pgps_create: " + self.lib.pgps_strerror(code).decode())
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            with self.lock:
                self.lib.pgps_destroy(self.handle)
                self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- knobs ---------------------------------------------------------------------------
    def _set(self, name, *values, optional=False):
        """One pgps_set_* / pgps_profile_* knob; `optional`: a library built before the knob leaves it alone."""
        if not optional or hasattr(self.lib, name):
            _facade.check(self, getattr(self.lib, name)(self.handle, *(int(v) for v in values)), name)

    def set_chunk(self, steps_per_lane):
        self._set("pgps_set_chunk", steps_per_lane)

    def set_stage(self, steps_per_subtile):
        """-1 auto, 0 direct global accesses, 2 / 4 steps per LDS-staged sub-tile."""
        self._set("pgps_set_stage", steps_per_subtile)

    def set_single_pass(self, mode=-1, window=0):
        """Single-pass filter kernel: -1 auto, 0 off, 1 on; window = look-back window in tiles (0 = keep)."""
        self._set("pgps_set_single_pass", mode, window)

    def set_family(self, family):
        """0 auto, 1 lane-chunk kernels (d <= 6), 2 wave-cooperative (any d <= 32), 3 row-cooperative (2 <= d <= 16), 4 quad-cooperative
        level-1 kernels (fp32, 5 <= d <= 8)."""
        self._set("pgps_set_family", family)

    def get_family(self, n_steps, d, f32=False, what=2):
        """PGPS_FAMILY_* code of the kernels a pkf (what = 0) / pks (1) / pkfs (2) / segment-phase (3) call will run on
        (1 lane-chunk 256 lanes, 11 lane-chunk 128 lanes, 2 wave-cooperative, 3 row-cooperative, 4 quad-cooperative, 5 two-rows);
        None with a library that cannot say."""
        if not hasattr(self.lib, "pgps_get_family"):
            return None
        fam = c_int(0)
        _facade.check(self, self.lib.pgps_get_family(self.handle, int(n_steps), int(d), 1 if f32 else 0, int(what), ctypes.byref(fam)),
                      "pgps_get_family")
        return fam.value

    def set_f32_policy(self, policy):
        """float32 series through a smoother (pkfs / pks): 0 = fp64 arithmetic on the float32 arrays where the grid is too
        dense for float32 arithmetic (probed per call on the device; always above d = 16), 1 = float32 arithmetic whatever
        the grid, 2 = always fp64 arithmetic.  `status()` & 4 tells whether a call was promoted."""
        if not hasattr(self.lib, "pgps_set_f32_policy"):
            raise RuntimeError("this libpgps has no pgps_set_f32_policy")
        self._set("pgps_set_f32_policy", policy)

    def set_block(self, lanes):
        """Lanes per workgroup of the lane-chunk kernels: 0 = automatic, 128, 256 (pgps_set_block)."""
        self._set("pgps_set_block", lanes)

    def set_dma(self, mode):
        """LDS-DMA ring in the Kalman pass (d = 2 fp64, 128-lane build): -1 automatic, 0 off, 1 on (pgps_set_dma)."""
        self._set("pgps_set_dma", mode, optional=True)

    def set_resident(self, mode):
        """Filter + smoother in ONE resident launch (fp64, d = 2, up to 4096 steps per CU): -1 automatic (from 2^17 steps),
        0 never, 1 wherever the series fits, 2 = 1 + in-kernel phase stamps (pgps_set_resident)."""
        self._set("pgps_set_resident", mode, optional=True)

    def set_shortcut(self, on):
        """Forgetting shortcut for the carry across workgroups (lane-chunk and resident kernels): 1 where it applies (default), 0 never."""
        self._set("pgps_set_shortcut", on, optional=True)

    def _stamps(self, name, width):
        n = c_int(0)
        fn = getattr(self.lib, name)
        _facade.check(self, fn(self.handle, None, 0, ctypes.byref(n)), name)
        out = np.zeros((max(n.value, 1), width), np.int64)
        _facade.check(self, fn(self.handle, _ptr(out), n.value, ctypes.byref(n)), name)
        return out[:n.value]

    def resident_stamps(self):
        """(workgroups, 16) cycle stamps of the last resident launch made under set_resident(2), and wall-clock stamps in
        slots 10 .. 13 when debug_resident_delay is armed (diagnostics)."""
        return self._stamps("pgps_resident_stamps", 16)

    def resident_wave_stamps(self):
        """(workgroups, 8) cycle stamps of the same launch as resident_stamps(): [k * 4 + wave] = the end of that wave's reduce
        (k = 0) / Kalman pass (k = 1)."""
        return self._stamps("pgps_resident_wave_stamps", 8)

    def debug_resident_delay(self, tile, phase=1, microseconds=200):
        """Diagnostics: workgroup `tile` of every following resident launch waits `microseconds` before it publishes its
        phase-1 / phase-2 total (spine records NaN-filled first); wall-clock stamps in slots 10 .. 13 of resident_stamps().
        tile = -1 disarms it (pgps_debug_resident_delay)."""
        self._set("pgps_debug_resident_delay", tile, phase, microseconds)

    def set_one_launch(self, max_steps):
        """Fused calls of short series in ONE launch up to max_steps steps: -1 automatic (2048 steps: kOneLaunchAuto), 0 never."""
        self._set("pgps_set_one_launch", max_steps, optional=True)

    def set_grad_pack(self, max_steps):
        """Gradient calls at d <= 2: one derivative direction per model up to this many steps (-1 automatic, 0 never)."""
        self._set("pgps_set_grad_pack", max_steps, optional=True)

    def set_batch_scratch(self, nbytes):
        """Scratch budget of the batched predict calls (pgps_gp_predict_batch_*): the models run in groups whose filtered
        moments and scan records fit it; 0 = the default.  A model's result does not depend on it."""
        self._set("pgps_set_batch_scratch", nbytes)

    def set_batch_form(self, form):
        """Launch form of the fused batched predict: 0 = automatic, 1 = one workgroup per model (one launch), 2 = three
        launches of (workgroups, models) grids."""
        self._set("pgps_set_batch_form", form)

    def set_rc_scan(self, mode):
        """Scans of the chain totals (row- / quad-cooperative families): -1 automatic, 0 one launch per level, 1 blocked."""
        self._set("pgps_set_rc_scan", mode, optional=True)

    def get_geometry(self, n, d):
        """(lanes per workgroup, steps per lane, workgroups) of a lane-chunk call of n steps at state dimension d <= 6."""
        lanes, lc, nb = c_int(0), c_int(0), c_int(0)
        _facade.check(self, self.lib.pgps_get_geometry(self.handle, int(n), int(d), ctypes.byref(lanes), ctypes.byref(lc),
                                                       ctypes.byref(nb)), "pgps_get_geometry")
        return lanes.value, lc.value, nb.value

    def get_chunk(self, n_steps):
        lc, nb = c_int(0), c_int(0)
        _facade.check(self, self.lib.pgps_get_chunk(self.handle, int(n_steps), ctypes.byref(lc), ctypes.byref(nb)),
                      "pgps_get_chunk")
        return lc.value, nb.value

    def get_batch_chunk(self, n_models, n_steps):
        """(steps per lane, workgroups per model) of a batched fused call of n_models models over n_steps steps (the merged
        steps of a predict): gp_ll_batch, the three-launch form of gp_predict_batch, the four-launch road of
        gp_ll_grad_adj_batch."""
        lc, nb = c_int(0), c_int(0)
        _facade.check(self, self.lib.pgps_get_batch_chunk(self.handle, int(n_models), int(n_steps), ctypes.byref(lc),
                                                          ctypes.byref(nb)), "pgps_get_batch_chunk")
        return lc.value, nb.value

    def get_panel_chunk(self, n_steps):
        """Steps per lane a panel launch (one workgroup per series) gives a series of n_steps steps, the merged steps of a
        predict: its own, or the pinned set_chunk where that covers the series."""
        lc = c_int(0)
        _facade.check(self, self.lib.pgps_get_panel_chunk(self.handle, int(n_steps), ctypes.byref(lc)), "pgps_get_panel_chunk")
        return lc.value

    def set_stream(self, hip_stream_handle):
        """Launch on an external hipStream_t (an integer handle; 0 / None = the HIP null stream)."""
        _facade.check(self, self.lib.pgps_set_stream(self.handle, c_void_p(hip_stream_handle or 0)), "pgps_set_stream")

    def use_own_stream(self):
        _facade.check(self, self.lib.pgps_use_own_stream(self.handle), "pgps_use_own_stream")

    def status(self):
        """Device-side diagnostic flags since the last call (0 = none); synchronises."""
        f = c_int(0)
        _facade.check(self, self.lib.pgps_status(self.handle, ctypes.byref(f)), "pgps_status")
        return f.value

    def synchronize(self):
        _facade.check(self, self.lib.pgps_synchronize(self.handle), "pgps_synchronize")

    def profile_enable(self, mask=0x7f):
        """mask: bit i = time every launch of kernel slot i (PGPS_K_*); 0 = off."""
        self._set("pgps_profile_enable", mask)

    def profile_sample(self, every_n):
        self._set("pgps_profile_sample", every_n)

    def profile_calibrate(self):
        """Mean elapsed ms of an empty hipEvent pair (the pair's own contribution to a timing)."""
        v = c_double(0.0)
        _facade.check(self, self.lib.pgps_profile_calibrate(self.handle, ctypes.byref(v)), "pgps_profile_calibrate")
        return v.value

    def profile_read(self, reset=True):
        k = 0                                   # slots of THIS library (PGPS_K_COUNT: 6 until round 4, 7 with the resident launch)
        while k < 16 and self.lib.pgps_kernel_name(k):
            k += 1
        ms = (c_double * 16)()
        cnt = (c_long * 16)()
        _facade.check(self, self.lib.pgps_profile_read(self.handle, ms, cnt, int(bool(reset))), "pgps_profile_read")
        return {self.lib.pgps_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(k)}

    # -- raw device memory -----------------------------------------------------------------
    def malloc(self, nbytes):
        p = c_void_p()
        with self.lock:
            _facade.check(self, self.lib.pgps_malloc(self.handle, int(nbytes), ctypes.byref(p)), "pgps_malloc")
        return p.value

    def free(self, ptr):
        with self.lock:
            _facade.check(self, self.lib.pgps_free(self.handle, c_void_p(ptr)), "pgps_free")

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        with self.lock:
            _facade.check(self, self.lib.pgps_memcpy_h2d(self.handle, c_void_p(dptr), arr.ctypes.data_as(c_void_p), arr.nbytes),
                          "pgps_memcpy_h2d")

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        with self.lock:
            _facade.check(self, self.lib.pgps_memcpy_d2h(self.handle, arr.ctypes.data_as(c_void_p), c_void_p(dptr), arr.nbytes),
                          "pgps_memcpy_d2h")

    # -- the communicator of a series sharded over GPUs (RCCL, owned by the context) -------------
    @staticmethod
    def comm_library():
        """Which RCCL libpgps uses -- loaded on first use: the copy already in the process (torch's, when
        torch.distributed's nccl backend is there) or the loader's librccl.so.1 -- or, prefixed with "unavailable: ", why
        there is none."""
        lib = load_library()
        if not hasattr(lib, "pgps_comm_library"):
            return "linked at build time"
        buf = ctypes.create_string_buffer(512)
        code = lib.pgps_comm_library(buf, 512)
        text = buf.value.decode(errors="replace")
        return text if code == 0 else "unavailable: " + text

    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from one rank, to be handed to every rank's comm_init (any transport: a file, MPI, a
        torch.distributed / TCP store ...)."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        code = load_library().pgps_comm_get_unique_id(buf)
        if code != PGPS_OK:
            raise PgpsError(code, "pgps_comm_get_unique_id")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique id must be {COMM_ID_BYTES} bytes")
        with self.lock:
            _facade.check(self, self.lib.pgps_comm_init(self.handle, ctypes.c_char_p(bytes(unique_id)), int(rank), int(nranks)),
                          "pgps_comm_init")

    def comm_destroy(self):
        with self.lock:
            _facade.check(self, self.lib.pgps_comm_destroy(self.handle), "pgps_comm_destroy")

    def comm_info(self):
        r, n = c_int(0), c_int(0)
        _facade.check(self, self.lib.pgps_comm_info(self.handle, ctypes.byref(r), ctypes.byref(n)), "pgps_comm_info")
        return r.value, n.value

    def comm_count(self):
        """(ranks, this rank) as RCCL itself reports them for the context's communicator (ncclCommCount /
        ncclCommUserRank); (0, 0) without a communicator."""
        n, r = c_int(0), c_int(0)
        if not hasattr(self.lib, "pgps_comm_count"):        # (a library built before round 3: A/B runs load those)
            return 0, 0
        _facade.check(self, self.lib.pgps_comm_count(self.handle, ctypes.byref(n), ctypes.byref(r)), "pgps_comm_count")
        return n.value, r.value

    # -- generic call by name ----------------------------------------------------------------
    def call(self, name, *args):
        with self.lock:
            _facade.check(self, getattr(self.lib, name)(self.handle, *args), name)


_contexts = {}
_ctx_lock = threading.Lock()


def get_context(device=0):
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = _contexts[device] = Context(device)
        return ctx
