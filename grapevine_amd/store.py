"""Host-side mirror of the store surface over libgvstore.so (ctypes).

`ObliviousStore.process_batch` is the batched form of the enclave handler's
QueryRequest -> QueryResponse dispatch (types/src/lib.rs:27-120,
api/proto/grapevine.proto:57-122); `access` is the single-op shim in the shape
of mc-oblivious-traits' ObliviousHashMap::access_and_insert.
There is no CPU fallback: if the HIP library or a GPU is missing, construction
fails loudly.
"""
import ctypes
import os

import numpy as np

from . import abi

_LIB = None
_HERE = os.path.dirname(os.path.abspath(__file__))
# The production library exports include/gvstore.h only; the test build adds
# the hooks of include/gvstore_test.h (dumps, raw stores).  Tests select it
# with GVS_TEST_HOOKS=1 (tests/conftest.py).
_LIB_PATH = os.path.join(_HERE, "libgvstore.so")
_TEST_LIB_PATH = os.path.join(_HERE, "libgvstore_test.so")

EXPORTED = (
    "gvs_config_init", "gvs_create", "gvs_destroy", "gvs_process_batch", "gvs_process_batches",
    "gvs_process_batch_device", "gvs_process_batches_device", "gvs_access", "gvs_get_stats",
    "gvs_synchronize", "gvs_set_option", "gvs_get_option", "gvs_set_timing", "gvs_last_timings", "gvs_last_error", "gvs_version",
    "gvs_comm_unique_id", "gvs_create_sharded", "gvs_storage_seal_row", "gvs_set_expiry_cutoff",
    "gvs_oram_create", "gvs_oram_destroy", "gvs_oram_access_batch", "gvs_oram_access_batch_device",
    "gvs_oram_set_timing", "gvs_oram_last_timings", "gvs_oram_last_error",
    "gvs_omap_create", "gvs_omap_destroy", "gvs_omap_access_batch", "gvs_omap_access_batch_device",
    "gvs_omap_set_timing", "gvs_omap_last_timings", "gvs_omap_last_error",
    "gvs_process_wire_batch", "gvs_process_wire_batch_device", "gvs_wire_decode_device",
    "gvs_wire_encode_device", "gvs_sr25519_verify", "gvs_sr25519_verify_device",
    "gvs_host_alloc", "gvs_host_free", "gvs_process_wire_batches",
    "gvs_ed25519_verify", "gvs_ed25519_verify_device",
    "gvs_challenge_derive", "gvs_challenge_derive_device", "gvs_process_wire_batch_seeded",
    "gvs_process_wire_batch_seeded_device", "gvs_process_wire_batches_seeded",
    "gvs_aead_open", "gvs_aead_open_device", "gvs_aead_seal", "gvs_aead_seal_device",
    "gvs_aead_open_long", "gvs_aead_open_long_device", "gvs_aead_seal_long", "gvs_aead_seal_long_device",
    "gvs_process_wire_batch_channel", "gvs_process_wire_batch_channel_device",
    "gvs_x25519", "gvs_x25519_device", "gvs_noise_hkdf", "gvs_noise_hkdf_device",
    "gvs_noise_ix_respond", "gvs_noise_ix_respond_device",
    "gvs_noise_ix_respond_long", "gvs_noise_ix_respond_long_device",
    "gvs_chachapoly_open", "gvs_chachapoly_open_device", "gvs_chachapoly_seal", "gvs_chachapoly_seal_device",
    "gvs_process_wire_batch_channel_cipher", "gvs_process_wire_batch_channel_cipher_device",
    "gvs_noise_ix_respond_cipher", "gvs_noise_ix_respond_cipher_device",
    "gvs_chachapoly_open_long", "gvs_chachapoly_open_long_device",
    "gvs_chachapoly_seal_long", "gvs_chachapoly_seal_long_device",
    "gvs_noise_ix_respond_long_cipher", "gvs_noise_ix_respond_long_cipher_device",
    "gvs_noise_ix_initiate", "gvs_noise_ix_initiate_device", "gvs_noise_ix_finish", "gvs_noise_ix_finish_device",
)
TEST_EXPORTED = ("gvs_dump_messages", "gvs_raw_size", "gvs_dump_raw", "gvs_store_raw",
                 "gvs_route_plan", "gvs_oram_test_handle", "gvs_omap_test_handle", "gvs_test_set_epoch")


def test_hooks_enabled():
    return os.environ.get("GVS_TEST_HOOKS") == "1"


class GvsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gvstore error {code}: {msg}")
        self.code = code


def load_library(path=None):
    """Load libgvstore.so and declare the C ABI signatures."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    # GVS_LIB_OVERRIDE: a diagnostic build of the same engine (tools/, A/B runs)
    p = path or os.environ.get("GVS_LIB_OVERRIDE") or (_TEST_LIB_PATH if test_hooks_enabled() else _LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError(f"{os.path.basename(p)} not built at {p}; run `make` (HIP extension missing)")
    lib = ctypes.CDLL(p)
    hooks = hasattr(lib, "gvs_dump_raw")
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.gvs_config_init.argtypes = [ctypes.POINTER(abi.GvsConfig), ctypes.c_uint64]
    lib.gvs_create.argtypes = [ctypes.POINTER(abi.GvsConfig), ctypes.POINTER(vp)]
    lib.gvs_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.gvs_create_sharded.argtypes = [ctypes.POINTER(abi.GvsConfig), ctypes.c_char_p,
                                       ctypes.POINTER(vp)]
    lib.gvs_destroy.argtypes = [vp]
    lib.gvs_process_batch.argtypes = [vp, vp, u32, vp]
    lib.gvs_process_batch_device.argtypes = [vp, vp, u32, vp]
    lib.gvs_process_batches_device.argtypes = [vp, vp, vp, u32, vp, ctypes.POINTER(u32)]
    lib.gvs_process_wire_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp, vp]
    lib.gvs_process_wire_batches.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp,
                                             ctypes.POINTER(u32)]
    lib.gvs_process_wire_batch_device.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp, vp]
    lib.gvs_process_wire_batch_seeded.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.gvs_process_wire_batches_seeded.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp,
                                                    vp, ctypes.POINTER(u32)]
    lib.gvs_process_wire_batch_seeded_device.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, vp, u32, vp, vp,
                                                         vp, vp]
    lib.gvs_process_wire_batch_channel.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32,
                                                   vp, vp, vp, vp]
    lib.gvs_process_wire_batch_channel_device.argtypes = lib.gvs_process_wire_batch_channel.argtypes
    lib.gvs_process_wire_batch_channel_cipher.argtypes = lib.gvs_process_wire_batch_channel_cipher_device.argtypes = \
        [vp, u32] + lib.gvs_process_wire_batch_channel.argtypes[1:]
    lib.gvs_aead_open.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, vp]
    lib.gvs_aead_open_device.argtypes = lib.gvs_aead_open.argtypes
    lib.gvs_aead_seal.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, u32, vp]
    lib.gvs_aead_seal_device.argtypes = lib.gvs_aead_seal.argtypes
    lib.gvs_aead_open_long.argtypes = lib.gvs_aead_open_long_device.argtypes = lib.gvs_aead_open.argtypes
    lib.gvs_aead_seal_long.argtypes = lib.gvs_aead_seal_long_device.argtypes = lib.gvs_aead_seal.argtypes
    lib.gvs_chachapoly_open.argtypes = lib.gvs_chachapoly_open_device.argtypes = lib.gvs_aead_open.argtypes
    lib.gvs_chachapoly_seal.argtypes = lib.gvs_chachapoly_seal_device.argtypes = lib.gvs_aead_seal.argtypes
    lib.gvs_chachapoly_open_long.argtypes = lib.gvs_chachapoly_open_long_device.argtypes = lib.gvs_aead_open.argtypes
    lib.gvs_chachapoly_seal_long.argtypes = lib.gvs_chachapoly_seal_long_device.argtypes = lib.gvs_aead_seal.argtypes
    lib.gvs_challenge_derive.argtypes = [vp, vp, vp, u32, vp]
    lib.gvs_challenge_derive_device.argtypes = [vp, vp, vp, u32, vp]
    lib.gvs_sr25519_verify.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp]
    lib.gvs_host_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.gvs_host_free.argtypes = [vp, vp]
    lib.gvs_sr25519_verify_device.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, vp, u32, vp]
    lib.gvs_ed25519_verify.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    lib.gvs_ed25519_verify_device.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, vp]
    lib.gvs_x25519.argtypes = [vp, vp, vp, u32, vp, vp]
    lib.gvs_x25519_device.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp]
    lib.gvs_noise_hkdf.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    lib.gvs_noise_hkdf_device.argtypes = [vp, vp, u32, vp, u32, u32, u32, vp, vp, u32]
    lib.gvs_noise_ix_respond.argtypes = abi.NOISE_IX_RESPOND_ARGTYPES
    lib.gvs_noise_ix_respond_device.argtypes = abi.NOISE_IX_RESPOND_ARGTYPES
    lib.gvs_noise_ix_respond_long.argtypes = abi.NOISE_IX_RESPOND_ARGTYPES
    lib.gvs_noise_ix_respond_long_device.argtypes = abi.NOISE_IX_RESPOND_ARGTYPES
    lib.gvs_noise_ix_respond_cipher.argtypes = lib.gvs_noise_ix_respond_cipher_device.argtypes = \
        [vp, u32] + abi.NOISE_IX_RESPOND_ARGTYPES[1:]
    lib.gvs_noise_ix_respond_long_cipher.argtypes = lib.gvs_noise_ix_respond_long_cipher_device.argtypes = \
        lib.gvs_noise_ix_respond_cipher.argtypes
    lib.gvs_noise_ix_initiate.argtypes = lib.gvs_noise_ix_initiate_device.argtypes = abi.NOISE_IX_INITIATE_ARGTYPES
    lib.gvs_noise_ix_finish.argtypes = lib.gvs_noise_ix_finish_device.argtypes = abi.NOISE_IX_FINISH_ARGTYPES
    lib.gvs_wire_decode_device.argtypes =[vp, vp, u32, vp, u32, vp, vp, vp, vp]
    lib.gvs_wire_encode_device.argtypes = [vp, vp, u32, vp, u32, vp]
    lib.gvs_process_batches.argtypes = [vp, vp, vp, u32, vp, ctypes.POINTER(u32)]
    lib.gvs_access.argtypes = [vp, vp, vp]
    lib.gvs_get_stats.argtypes = [vp, ctypes.POINTER(abi.GvsStats)]
    lib.gvs_synchronize.argtypes = [vp]
    lib.gvs_set_timing.argtypes = [vp, i32]
    lib.gvs_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    lib.gvs_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    lib.gvs_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p),
                                     ctypes.POINTER(ctypes.c_float), i32]
    cp, u64 = ctypes.c_char_p, ctypes.c_uint64
    lib.gvs_storage_seal_row.argtypes = [cp, u32, u64, u32, cp, cp, cp, cp, cp]
    if hooks:
        lib.gvs_dump_messages.argtypes = [vp, vp, ctypes.c_uint64]
        lib.gvs_raw_size.argtypes = [vp, u32, u32, ctypes.POINTER(u64)]
        lib.gvs_dump_raw.argtypes = [vp, u32, u32, u64, vp, u64]
        lib.gvs_store_raw.argtypes = [vp, u32, u32, u64, vp, u64]
        P32 = ctypes.POINTER(u32)
        lib.gvs_route_plan.argtypes = [ctypes.POINTER(abi.GvsConfig), vp, u32, vp, P32, P32, vp]
        lib.gvs_oram_test_handle.argtypes = [vp]
        lib.gvs_oram_test_handle.restype = vp
        lib.gvs_omap_test_handle.argtypes = [vp]
        lib.gvs_omap_test_handle.restype = vp
        lib.gvs_test_set_epoch.argtypes = [vp, u32]
    lib.gvs_last_error.argtypes = [vp]
    lib.gvs_set_expiry_cutoff.argtypes = [vp, ctypes.c_uint64]
    lib.gvs_last_error.restype = ctypes.c_char_p
    lib.gvs_version.restype = ctypes.c_char_p
    lib.gvs_oram_create.argtypes = [ctypes.POINTER(abi.GvsOramConfig), ctypes.POINTER(vp)]
    lib.gvs_oram_destroy.argtypes = [vp]
    lib.gvs_oram_access_batch.argtypes = [vp, vp, u32, vp]
    lib.gvs_oram_access_batch_device.argtypes = [vp, vp, u32, vp]
    lib.gvs_oram_set_timing.argtypes = [vp, i32]
    lib.gvs_oram_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(ctypes.c_float), i32]
    lib.gvs_oram_last_error.argtypes = [vp]
    lib.gvs_oram_last_error.restype = ctypes.c_char_p
    lib.gvs_omap_create.argtypes = [ctypes.POINTER(abi.GvsOramConfig), ctypes.POINTER(vp)]
    lib.gvs_omap_destroy.argtypes = [vp]
    lib.gvs_omap_access_batch.argtypes = [vp, vp, u32, vp]
    lib.gvs_omap_access_batch_device.argtypes = [vp, vp, u32, vp]
    lib.gvs_omap_set_timing.argtypes = [vp, i32]
    lib.gvs_omap_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(ctypes.c_float), i32]
    lib.gvs_omap_last_error.argtypes = [vp]
    lib.gvs_omap_last_error.restype = ctypes.c_char_p
    for name in EXPORTED + (TEST_EXPORTED if hooks else ()):
        if name not in ("gvs_last_error", "gvs_version", "gvs_oram_last_error", "gvs_omap_last_error",
                        "gvs_oram_test_handle", "gvs_omap_test_handle"):
            getattr(lib, name).restype = i32
    if path is None:
        _LIB = lib
    return lib


def route_plan(config, reqs, with_shed=False):
    """The router's placement of one source's batch, on the host (test
    library, gvs_route_plan): -> (slot per request, C, shard pipeline size,
    overflowed[, shed flags])."""
    lib = load_library(_TEST_LIB_PATH)
    reqs = np.ascontiguousarray(reqs, dtype=abi.REQUEST_DTYPE)
    slot = np.zeros(len(reqs), dtype=np.uint32)
    shed = np.zeros(len(reqs), dtype=np.uint8)
    cap, be = ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib.gvs_route_plan(ctypes.byref(config), reqs.ctypes.data, len(reqs), slot.ctypes.data,
                            ctypes.byref(cap), ctypes.byref(be), shed.ctypes.data)
    if rc not in (0, abi.GVS_ERR_BATCH_OVERFLOW):
        raise GvsError(rc, "gvs_route_plan failed")
    out = (slot, cap.value, be.value, rc == abi.GVS_ERR_BATCH_OVERFLOW)
    return out + (shed.astype(bool),) if with_shed else out


def comm_unique_id():
    """RCCL unique id for gvs_create_sharded (call on one rank, share with all)."""
    buf = ctypes.create_string_buffer(abi.COMM_ID_BYTES)
    rc = load_library().gvs_comm_unique_id(buf)
    if rc != 0:
        raise GvsError(rc, "gvs_comm_unique_id failed")
    return buf.raw


class ObliviousStore:
    """One store handle (not thread-safe, like `&mut self`).

    - `comm_id=None`, `config.shard_count <= 1`: one shard on one GPU.
    - `comm_id=None`, `config.shard_count = S > 1`: all S shards on
      `config.device` in this process (single-GPU test form of the sharded
      store; a batch is the concatenation of S sources' batches).
    - `comm_id` given: this process's shard `config.shard_index` of an
      S-process store over RCCL; every call is collective.
    """

    def __init__(self, config, comm_id=None):
        self.lib = load_library()
        self.config = config
        self._pinned = []
        h = ctypes.c_void_p()
        if comm_id is None:
            rc = self.lib.gvs_create(ctypes.byref(config), ctypes.byref(h))
        else:
            rc = self.lib.gvs_create_sharded(ctypes.byref(config), comm_id, ctypes.byref(h))
        if rc != 0:
            raise GvsError(rc, "gvs_create failed (no GPU, bad config or out of memory)")
        self.h = h
        self.B = config.max_batch

    def close(self):
        if getattr(self, "h", None):
            for p in getattr(self, "_pinned", []):
                self.lib.gvs_host_free(self.h, p)
            self._pinned = []
            self.lib.gvs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise GvsError(rc, self.lib.gvs_last_error(self.h).decode())

    def process_batch(self, reqs):
        """reqs: np.ndarray of abi.REQUEST_DTYPE -> responses (abi.RESPONSE_DTYPE)."""
        reqs = np.ascontiguousarray(reqs, dtype=abi.REQUEST_DTYPE)
        out = np.zeros(len(reqs), dtype=abi.RESPONSE_DTYPE)
        self._check(self.lib.gvs_process_batch(self.h, reqs.ctypes.data, len(reqs), out.ctypes.data))
        return out

    def process_batches(self, batches):
        """Several batches from host memory, double-buffered (gvs_process_batches).
        -> list of response arrays.  On a failing batch raises GvsError with
        `.applied` = the number of batches applied before it."""
        counts = np.array([len(b) for b in batches], dtype=np.uint32)
        reqs = np.ascontiguousarray(np.concatenate(batches) if len(batches) else
                                    np.zeros(0, dtype=abi.REQUEST_DTYPE), dtype=abi.REQUEST_DTYPE)
        out = np.zeros(len(reqs), dtype=abi.RESPONSE_DTYPE)
        applied = ctypes.c_uint32(0)
        rc = self.lib.gvs_process_batches(self.h, reqs.ctypes.data, counts.ctypes.data, len(counts),
                                          out.ctypes.data, ctypes.byref(applied))
        if rc != 0:
            err = GvsError(rc, (self.lib.gvs_last_error(self.h) or b"").decode())
            err.applied = applied.value
            raise err
        return np.split(out, np.cumsum(counts)[:-1]) if len(counts) else []

    def process_batch_device(self, d_reqs_ptr, n, d_out_ptr):
        self._check(self.lib.gvs_process_batch_device(self.h, d_reqs_ptr, n, d_out_ptr))

    def process_batches_device(self, d_reqs_ptr, counts, d_out_ptr):
        """k batches from device memory in one call (gvs_process_batches_device):
        every batch enqueued before any result is awaited.  Returns the number
        applied; raises GvsError (with .applied) at the first failing batch."""
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        applied = ctypes.c_uint32(0)
        rc = self.lib.gvs_process_batches_device(self.h, d_reqs_ptr, c.ctypes.data, len(c), d_out_ptr,
                                                 ctypes.byref(applied))
        if rc != 0:
            err = GvsError(rc, self.lib.gvs_last_error(self.h).decode())
            err.applied = applied.value
            raise err
        return applied.value

    @staticmethod
    def _wire_slab(msgs, in_stride):
        if isinstance(msgs, np.ndarray):
            n, width = msgs.shape
            lens = np.full(n, width, np.uint32)
            stride = in_stride or width
            slab = np.zeros((n, stride), np.uint8)
            slab[:, :width] = msgs
        else:
            n = len(msgs)
            lens = np.array([len(m) for m in msgs], np.uint32)
            stride = in_stride or max(int(lens.max()) if n else 1, 1)
            slab = np.zeros((n, stride), np.uint8)
            for k, m in enumerate(msgs):
                slab[k, :len(m)] = np.frombuffer(bytes(m), np.uint8)
        return slab, lens, stride

    def process_wire_batches(self, batches, times, in_stride=None,
                             out_stride=abi.WIRE_RESPONSE_BYTES, challenges=None):
        """Several wire batches in one double-buffered call
        (gvs_process_wire_batches).  batches: list of lists of message bytes;
        times / challenges: per message over all batches (times may be a
        scalar).  -> list of (response bytes list, status array) per batch.
        On a failing batch raises GvsError with `.applied`."""
        counts = np.array([len(b) for b in batches], dtype=np.uint32)
        flat = [m for b in batches for m in b]
        n = len(flat)
        slab, lens, stride = self._wire_slab(flat, in_stride)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.uint64), (n,)))
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint32)
        chal = None
        if challenges is not None:
            chal = np.ascontiguousarray(challenges, np.uint8).reshape(n, 32)
        applied = ctypes.c_uint32(0)
        rc = self.lib.gvs_process_wire_batches(
            self.h, slab.ctypes.data, stride, lens.ctypes.data, counts.ctypes.data, len(counts),
            times.ctypes.data, chal.ctypes.data if chal is not None else None, out.ctypes.data,
            out_stride, out_lens.ctypes.data, status.ctypes.data, ctypes.byref(applied))
        if rc != 0:
            err = GvsError(rc, (self.lib.gvs_last_error(self.h) or b"").decode())
            err.applied = applied.value
            raise err
        res, o = [], 0
        for c in counts:
            res.append(([out[k, :out_lens[k]].tobytes() for k in range(o, o + c)], status[o:o + c]))
            o += int(c)
        return res

    def process_wire_batch(self, msgs, times, in_stride=None, out_stride=abi.WIRE_RESPONSE_BYTES,
                           challenges=None):
        """Wire QueryRequests (list of bytes, or an (n, L) uint8 array of
        canonical messages) through the device codec and the store
        (gvs_process_wire_batch).  `challenges` ((n, 32) uint8, optional): the
        challenge each auth_signature must sign; failing requests become hard
        errors.  -> (list of response bytes, (n, 64) signatures, per-request
        GVS_WIRE_* status).  A hard error's response is b"" (the handler
        answers it with a gRPC error)."""
        slab, lens, stride = self._wire_slab(msgs, in_stride)
        n = len(lens)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.uint64), (n,)))
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        sigs = np.zeros((n, 64), np.uint8)
        status = np.zeros(n, np.uint32)
        chal = None
        if challenges is not None:
            chal = np.ascontiguousarray(challenges, np.uint8).reshape(n, 32)
        self._check(self.lib.gvs_process_wire_batch(
            self.h, slab.ctypes.data, stride, lens.ctypes.data, n, times.ctypes.data,
            chal.ctypes.data if chal is not None else None, out.ctypes.data, out_stride,
            out_lens.ctypes.data, sigs.ctypes.data, status.ctypes.data))
        return [out[k, :out_lens[k]].tobytes() for k in range(n)], sigs, status

    @staticmethod
    def _seeds_draws(seeds, draws, n):
        """(n, 32) uint8 seeds and (n,) uint64 draw indices, or (None, None);
        one without the other is passed on for the library to refuse."""
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint8).reshape(n, 32)
        if draws is not None:
            draws = np.ascontiguousarray(draws, np.uint64).reshape(n)
        return seeds, draws

    def process_wire_batch_seeded(self, msgs, times, seeds, draws, in_stride=None,
                                  out_stride=abi.WIRE_RESPONSE_BYTES):
        """process_wire_batch with the challenges derived on the device
        (gvs_process_wire_batch_seeded): request k must sign draw number
        draws[k] of ChaCha20Rng(seeds[k]) (`challenge_derive`).  seeds (n, 32)
        uint8 and draws (n,) uint64, or both None (no check).  -> (list of
        response bytes, (n, 64) signatures, per-request GVS_WIRE_* status,
        (n, 32) derived challenges; zero when nothing was derived)."""
        slab, lens, stride = self._wire_slab(msgs, in_stride)
        n = len(lens)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.uint64), (n,)))
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        sigs = np.zeros((n, 64), np.uint8)
        status = np.zeros(n, np.uint32)
        chal = np.zeros((n, 32), np.uint8)
        seeds, draws = self._seeds_draws(seeds, draws, n)
        self._check(self.lib.gvs_process_wire_batch_seeded(
            self.h, slab.ctypes.data, stride, lens.ctypes.data, n, times.ctypes.data,
            seeds.ctypes.data if seeds is not None else None,
            draws.ctypes.data if draws is not None else None, out.ctypes.data, out_stride,
            out_lens.ctypes.data, sigs.ctypes.data, status.ctypes.data, chal.ctypes.data))
        return [out[k, :out_lens[k]].tobytes() for k in range(n)], sigs, status, chal

    def process_wire_batches_seeded(self, batches, times, seeds, draws, in_stride=None,
                                    out_stride=abi.WIRE_RESPONSE_BYTES):
        """process_wire_batches with the challenges derived on the device
        (gvs_process_wire_batches_seeded); seeds / draws per message over all
        batches.  -> list of (response bytes list, status array, (c, 32)
        derived challenges) per batch.  On a failing batch raises GvsError
        with `.applied`."""
        counts = np.array([len(b) for b in batches], dtype=np.uint32)
        flat = [m for b in batches for m in b]
        n = len(flat)
        slab, lens, stride = self._wire_slab(flat, in_stride)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.uint64), (n,)))
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint32)
        chal = np.zeros((n, 32), np.uint8)
        seeds, draws = self._seeds_draws(seeds, draws, n)
        applied = ctypes.c_uint32(0)
        rc = self.lib.gvs_process_wire_batches_seeded(
            self.h, slab.ctypes.data, stride, lens.ctypes.data, counts.ctypes.data, len(counts),
            times.ctypes.data, seeds.ctypes.data if seeds is not None else None,
            draws.ctypes.data if draws is not None else None, out.ctypes.data, out_stride,
            out_lens.ctypes.data, status.ctypes.data, chal.ctypes.data, ctypes.byref(applied))
        if rc != 0:
            err = GvsError(rc, (self.lib.gvs_last_error(self.h) or b"").decode())
            err.applied = applied.value
            raise err
        res, o = [], 0
        for c in counts:
            res.append(([out[k, :out_lens[k]].tobytes() for k in range(o, o + c)], status[o:o + c],
                        chal[o:o + c]))
            o += int(c)
        return res

    def process_wire_batch_channel(self, msgs, times, seeds, draws, open_keys, open_ivs, seal_keys,
                                   seal_ivs, in_stride=None, out_stride=None, cipher=None):
        """process_wire_batch_seeded behind the channel cipher
        (gvs_process_wire_batch_channel): msgs are the requests as ciphertext
        | tag under open_keys[k] (n, 32) / open_ivs[k] (n, 12, `abi.noise_iv`),
        and the responses come back as ciphertext | tag under seal_keys[k] /
        seal_ivs[k].  A request whose tag fails answers b"" with status
        WIRE_BAD_CHANNEL_TAG.  cipher: abi.CIPHER_AESGCM or
        abi.CIPHER_CHACHAPOLY (nonces from `abi.noise_nonce_chachapoly`)
        through gvs_process_wire_batch_channel_cipher; None is the call
        above.  -> what process_wire_batch_seeded returns."""
        if in_stride is None:
            in_stride = -(-max([len(m) for m in msgs] + [1]) // 16) * 16
        if out_stride is None:
            out_stride = -(-(abi.WIRE_RESPONSE_BYTES + abi.AEAD_TAG_BYTES) // 16) * 16
        slab, lens, stride = self._wire_slab(msgs, in_stride)
        n = len(lens)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.uint64), (n,)))
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        sigs = np.zeros((n, 64), np.uint8)
        status = np.zeros(n, np.uint32)
        chal = np.zeros((n, 32), np.uint8)
        seeds, draws = self._seeds_draws(seeds, draws, n)
        keys = [np.ascontiguousarray(a, np.uint8).reshape(n, w)
                for a, w in ((open_keys, 32), (open_ivs, 12), (seal_keys, 32), (seal_ivs, 12))]
        fn, head = self.lib.gvs_process_wire_batch_channel, [self.h]
        if cipher is not None:
            fn, head = self.lib.gvs_process_wire_batch_channel_cipher, [self.h, cipher]
        self._check(fn(
            *head, slab.ctypes.data, stride, lens.ctypes.data, n, times.ctypes.data,
            seeds.ctypes.data if seeds is not None else None,
            draws.ctypes.data if draws is not None else None, *[a.ctypes.data for a in keys],
            out.ctypes.data, out_stride, out_lens.ctypes.data, sigs.ctypes.data, status.ctypes.data,
            chal.ctypes.data))
        return [out[k, :out_lens[k]].tobytes() for k in range(n)], sigs, status, chal

    def _aead(self, seal, keys, ivs, msgs, aads, long=False, name="gvs_aead"):
        n = len(msgs)
        keys = np.ascontiguousarray(keys, np.uint8).reshape(n, 32)
        ivs = np.ascontiguousarray(ivs, np.uint8).reshape(n, 12)
        pad16 = lambda v: -(-max(v, 1) // 16) * 16
        slab, lens, stride = self._wire_slab(msgs, pad16(max([len(m) for m in msgs] + [0])))
        aad = aad_lens = None
        aad_stride = 16
        if aads is not None:
            aad, aad_lens, aad_stride = self._wire_slab(aads, pad16(max([len(a) for a in aads] + [0])))
        out_stride = stride + 16 if seal else stride
        out = np.zeros((n, out_stride), np.uint8)
        out_lens = np.zeros(n, np.uint32)
        ok = np.ones(n, np.uint32)
        fn = getattr(self.lib, name + ("_seal" if seal else "_open") + ("_long" if long else ""))
        self._check(fn(self.h, keys.ctypes.data, ivs.ctypes.data,
                       aad.ctypes.data if aad is not None else None, aad_stride,
                       aad_lens.ctypes.data if aad is not None else None, slab.ctypes.data, stride,
                       lens.ctypes.data, n, out.ctypes.data, out_stride, out_lens.ctypes.data,
                       *([] if seal else [ok.ctypes.data])))
        return out, out_lens, ok.astype(bool)

    def aead_seal(self, keys, ivs, msgs, aads=None):
        """Batched AES-256-GCM sealing on the device (gvs_aead_seal): keys
        (n, 32) and ivs (n, 12) uint8, msgs a list of n plaintexts, aads an
        optional list of n byte strings -> list of ciphertext | tag."""
        out, out_lens, _ = self._aead(True, keys, ivs, msgs, aads)
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))]

    def aead_open(self, keys, ivs, msgs, aads=None):
        """Batched AES-256-GCM opening on the device (gvs_aead_open): msgs a
        list of n ciphertext | tag -> (list of plaintexts, (n,) bool verdicts,
        the (n, stride) output slab); a message that does not verify is b""
        and its slot all zero."""
        out, out_lens, ok = self._aead(False, keys, ivs, msgs, aads)
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))], ok, out

    def aead_seal_long(self, keys, ivs, msgs, aads=None):
        """aead_seal for whole Noise messages (gvs_aead_seal_long): plaintexts
        of up to abi.AEAD_LONG_TEXT_MAX bytes, one workgroup per message."""
        out, out_lens, _ = self._aead(True, keys, ivs, msgs, aads, long=True)
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))]

    def aead_open_long(self, keys, ivs, msgs, aads=None):
        """aead_open for whole Noise messages (gvs_aead_open_long): ciphertext
        | tag of up to 65 535 bytes -> (plaintexts, verdicts, output slab)."""
        out, out_lens, ok = self._aead(False, keys, ivs, msgs, aads, long=True)
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))], ok, out

    def chachapoly_seal(self, keys, nonces, msgs, aads=None):
        """aead_seal with ChaCha20-Poly1305 (gvs_chachapoly_seal): the same
        arguments, nonces (n, 12) where it takes ivs."""
        out, out_lens, _ = self._aead(True, keys, nonces, msgs, aads, name="gvs_chachapoly")
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))]

    def chachapoly_open(self, keys, nonces, msgs, aads=None):
        """aead_open with ChaCha20-Poly1305 (gvs_chachapoly_open) ->
        (plaintexts, verdicts, output slab)."""
        out, out_lens, ok = self._aead(False, keys, nonces, msgs, aads, name="gvs_chachapoly")
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))], ok, out

    def chachapoly_seal_long(self, keys, nonces, msgs, aads=None):
        """chachapoly_seal for whole Noise messages (gvs_chachapoly_seal_long):
        plaintexts of up to abi.AEAD_LONG_TEXT_MAX bytes, one workgroup per message."""
        out, out_lens, _ = self._aead(True, keys, nonces, msgs, aads, long=True, name="gvs_chachapoly")
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))]

    def chachapoly_open_long(self, keys, nonces, msgs, aads=None):
        """chachapoly_open for whole Noise messages (gvs_chachapoly_open_long):
        ciphertext | tag of up to 65 535 bytes -> (plaintexts, verdicts, output slab)."""
        out, out_lens, ok = self._aead(False, keys, nonces, msgs, aads, long=True, name="gvs_chachapoly")
        return [out[k, :out_lens[k]].tobytes() for k in range(len(msgs))], ok, out

    def challenge_derive(self, seeds, draws):
        """The challenge stream on the device (gvs_challenge_derive): seeds
        (n, 32) uint8, draws (n,) uint64 -> (n, 32) uint8, row k = draw number
        draws[k] of ChaCha20Rng(seeds[k])."""
        draws = np.ascontiguousarray(draws, np.uint64).reshape(-1)
        n = len(draws)
        seeds = np.ascontiguousarray(seeds, np.uint8).reshape(n, 32)
        out = np.zeros((n, 32), np.uint8)
        self._check(self.lib.gvs_challenge_derive(self.h, seeds.ctypes.data, draws.ctypes.data, n,
                                                  out.ctypes.data))
        return out

    def host_array(self, count, dtype):
        """A numpy array of `count` items in pinned host memory (gvs_host_alloc),
        which gvs_process_batches copies without staging.  Freed when the
        store closes."""
        dtype = np.dtype(dtype)
        p = ctypes.c_void_p()
        self._check(self.lib.gvs_host_alloc(self.h, max(1, count * dtype.itemsize), ctypes.byref(p)))
        self._pinned.append(p)
        buf = (ctypes.c_uint8 * (count * dtype.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=count)

    def sr25519_verify(self, pks, msgs, sigs, context=b"grapevine-challenge"):
        """Batched schnorrkel verification on the device (gvs_sr25519_verify):
        pks (n, 32), msgs (n, L), sigs (n, 64) uint8 -> (n,) bool."""
        pks = np.ascontiguousarray(pks, np.uint8)
        msgs = np.ascontiguousarray(msgs, np.uint8)
        sigs = np.ascontiguousarray(sigs, np.uint8)
        n = len(pks)
        ok = np.zeros(n, np.uint32)
        self._check(self.lib.gvs_sr25519_verify(self.h, pks.ctypes.data, msgs.ctypes.data,
                                                msgs.shape[1] if msgs.ndim == 2 else 0,
                                                sigs.ctypes.data, n, context, len(context),
                                                ok.ctypes.data))
        return ok.astype(bool)

    def ed25519_verify(self, pks, msgs, sigs):
        """Batched Ed25519 verification on the device (gvs_ed25519_verify; RFC
        8032 strict decoding, cofactorless): pks (n, 32), msgs (n, L), sigs
        (n, 64) uint8 -> (n,) bool."""
        pks = np.ascontiguousarray(pks, np.uint8)
        msgs = np.ascontiguousarray(msgs, np.uint8)
        sigs = np.ascontiguousarray(sigs, np.uint8)
        n = len(pks)
        ok = np.zeros(n, np.uint32)
        self._check(self.lib.gvs_ed25519_verify(self.h, pks.ctypes.data, msgs.ctypes.data,
                                                msgs.shape[1] if msgs.ndim == 2 else 0,
                                                sigs.ctypes.data, n, ok.ctypes.data))
        return ok.astype(bool)

    def x25519(self, scalars, points=None):
        """Batched X25519 on the device (gvs_x25519; RFC 7748): scalars (n, 32)
        uint8, points (n, 32) uint8 or None for the base point -> ((n, 32)
        uint8 results, (n,) bool: False where the result is all zero)."""
        scalars = np.ascontiguousarray(scalars, np.uint8).reshape(-1, 32)
        n = len(scalars)
        if points is not None:
            points = np.ascontiguousarray(points, np.uint8).reshape(n, 32)
        out = np.zeros((n, 32), np.uint8)
        ok = np.zeros(n, np.uint32)
        self._check(self.lib.gvs_x25519(self.h, scalars.ctypes.data,
                                        points.ctypes.data if points is not None else None, n,
                                        out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def noise_hkdf(self, cks, ikm=None):
        """Batched Noise HKDF-SHA-512 on the device (gvs_noise_hkdf): cks
        (n, 64) uint8, ikm (n, 32) uint8 (MixKey of DH outputs) or None
        (Split) -> two (n, 64) uint8 outputs."""
        cks = np.ascontiguousarray(cks, np.uint8).reshape(-1, 64)
        n = len(cks)
        if ikm is not None:
            ikm = np.ascontiguousarray(ikm, np.uint8).reshape(n, 32)
        out1, out2 = np.zeros((n, 64), np.uint8), np.zeros((n, 64), np.uint8)
        self._check(self.lib.gvs_noise_hkdf(self.h, cks.ctypes.data,
                                            ikm.ctypes.data if ikm is not None else None,
                                            32 if ikm is not None else 0, n, out1.ctypes.data,
                                            out2.ctypes.data))
        return out1, out2

    def noise_ix_respond(self, static_secret, ephemerals, msg1, payload=b"", prologue=b"",
                         msg2_stride=None, cipher=None):
        """The responder's side of n Noise_IX_25519_AESGCM_SHA512 handshakes
        on the device (gvs_noise_ix_respond): static_secret 32 bytes,
        ephemerals (n, 32) fresh secrets, msg1 a list of n first messages,
        payload one byte string for all or a list of n of one length, prologue
        bytes -> (list of n second messages, recv_keys (n, 32), send_keys
        (n, 32), hashes (n, 64), (n,) bool, the (n, stride) message-2 slab).  A
        handshake that fails is b"" with zero keys and hash.  cipher:
        abi.CIPHER_AESGCM or abi.CIPHER_CHACHAPOLY
        (Noise_IX_25519_ChaChaPoly_SHA512) through gvs_noise_ix_respond_cipher;
        None is the call above.  The form on torch tensors is
        `noise_ix_respond_device`."""
        fn = self.lib.gvs_noise_ix_respond
        if cipher is not None:
            fn = lambda h, *rest: self.lib.gvs_noise_ix_respond_cipher(h, cipher, *rest)
        return self._noise_ix_respond(fn, 1, static_secret, ephemerals, msg1,
                                      payload, prologue, msg2_stride)

    def noise_ix_respond_long(self, static_secret, ephemerals, msg1, payload=b"", prologue=b"",
                              msg2_stride=None, cipher=None):
        """noise_ix_respond with a payload of up to abi.NOISE_PAYLOAD2_LONG_MAX
        bytes inside message 2 (gvs_noise_ix_respond_long): the same arguments
        and results; msg2_stride is a multiple of 16 (default: 96 + the
        payload's length, rounded up).  cipher: as in noise_ix_respond, through
        gvs_noise_ix_respond_long_cipher; None is the call above.  The form on
        torch tensors is `noise_ix_respond_long_device`."""
        fn = self.lib.gvs_noise_ix_respond_long
        if cipher is not None:
            fn = lambda h, *rest: self.lib.gvs_noise_ix_respond_long_cipher(h, cipher, *rest)
        return self._noise_ix_respond(fn, 16, static_secret, ephemerals, msg1, payload, prologue, msg2_stride)

    def _noise_ix_respond(self, fn, align, static_secret, ephemerals, msg1, payload, prologue, msg2_stride):
        """The host forms: payload rows and the default message-2 stride are
        rounded up to `align` bytes."""
        up = lambda v: -(-v // align) * align
        n = len(msg1)
        eph = np.ascontiguousarray(ephemerals, np.uint8).reshape(n, 32)
        slab, lens, stride = self._wire_slab(msg1, max([len(m) for m in msg1] + [64]))
        one = isinstance(payload, (bytes, bytearray))
        pays = [bytes(payload)] if one else [bytes(p) for p in payload]
        p2 = len(pays[0]) if pays else 0
        if any(len(p) != p2 for p in pays) or (not one and len(pays) != n):
            raise ValueError("noise_ix_respond: one payload length per call")
        pay = np.frombuffer(b"".join(p.ljust(up(p2), b"\0") for p in pays), np.uint8) if p2 else None
        m2s = msg2_stride if msg2_stride is not None else up(96 + p2)
        msg2 = np.zeros((n, max(m2s, 1)), np.uint8)
        m2l, ok = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        rk, sk, hh = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
        self._check(fn(
            self.h, bytes(static_secret), bytes(prologue), len(prologue), eph.ctypes.data, slab.ctypes.data,
            stride, lens.ctypes.data, pay.ctypes.data if pay is not None else None, 0 if one else up(p2), p2, n,
            msg2.ctypes.data, m2s, m2l.ctypes.data, rk.ctypes.data, sk.ctypes.data, hh.ctypes.data,
            ok.ctypes.data))
        return [msg2[k, :m2l[k]].tobytes() for k in range(n)], rk, sk, hh, ok.astype(bool), msg2

    def noise_ix_respond_device(self, static_secret, ephemerals, msg1, msg1_lens, payload, payload_len,
                                msg2, msg2_lens, recv_keys, send_keys, hashes, ok, prologue=b"", long=False,
                                cipher=None):
        """gvs_noise_ix_respond_device on torch CUDA tensors: ephemerals
        (n, >= 32 contiguous 32), msg1 (n, stride) uint8, msg1_lens (n,) int32,
        payload (n, stride) uint8, a 1-D tensor (one payload for all) or None,
        and the outputs msg2 (n, stride) uint8, msg2_lens (n,) int32,
        recv_keys / send_keys (n, 32), hashes (n, 64) or None, ok (n,) int32,
        all written in place.  The caller synchronises its own streams first.
        long: gvs_noise_ix_respond_long_device, whose payload and msg2 rows are
        16-byte aligned, with strides that are multiples of 16.  cipher:
        gvs_noise_ix_respond_cipher_device, or with long
        gvs_noise_ix_respond_long_cipher_device."""
        n = msg1.shape[0]
        ptr = lambda t: t.data_ptr() if t is not None else None
        pstride = 0 if payload is None or payload.dim() == 1 else payload.stride(0)
        fn, head = self.lib.gvs_noise_ix_respond_long_device if long else self.lib.gvs_noise_ix_respond_device, [self.h]
        if cipher is not None:
            fn = self.lib.gvs_noise_ix_respond_long_cipher_device if long else self.lib.gvs_noise_ix_respond_cipher_device
            head = [self.h, cipher]
        self._check(fn(
            *head, bytes(static_secret), bytes(prologue), len(prologue), ptr(ephemerals), ptr(msg1),
            msg1.stride(0), ptr(msg1_lens), ptr(payload), pstride, payload_len, n, ptr(msg2), msg2.stride(0),
            ptr(msg2_lens), ptr(recv_keys), ptr(send_keys), ptr(hashes), ptr(ok)))

    def noise_ix_respond_long_device(self, *args, **kw):
        """noise_ix_respond_device(..., long=True)."""
        self.noise_ix_respond_device(*args, long=True, **kw)

    def noise_ix_initiate(self, statics, ephemerals, payload=b"", prologue=b"", msg1_stride=None, cipher=None,
                          device=False, out=None):
        """The initiator's message 1 of n Noise IX handshakes on the device
        (gvs_noise_ix_initiate): statics 32 bytes (one static secret for all)
        or (n, 32), ephemerals (n, 32) fresh secrets, payload one byte string
        for all or a list of n of one length (<= abi.NOISE_PAYLOAD1_MAX),
        prologue bytes -> (list of n first messages, states (n, 64), the
        (n, stride) message-1 slab).  cipher: abi.CIPHER_AESGCM (None) or
        abi.CIPHER_CHACHAPOLY.  device=True is gvs_noise_ix_initiate_device on
        torch CUDA tensors: statics (32,) or (n, >= 32), ephemerals (n, 32),
        payload None, 1-D (one for all) or (n, >= its length); out = (msg1
        (n, stride) uint8, msg1_lens (n,) int32, states (n, 64)) is written in
        place (made when None) and returned; the caller synchronises its own
        streams first."""
        cipher = abi.CIPHER_AESGCM if cipher is None else cipher
        if device:
            import torch
            n = ephemerals.shape[0]
            plen = 0 if payload is None else payload.shape[-1]
            if out is None:
                kw = dict(device=ephemerals.device)
                out = (torch.zeros((n, msg1_stride or 64 + plen), dtype=torch.uint8, **kw),
                       torch.zeros(n, dtype=torch.int32, **kw), torch.zeros((n, 64), dtype=torch.uint8, **kw))
            msg1, lens, states = out
            self._check(self.lib.gvs_noise_ix_initiate_device(
                self.h, cipher, bytes(prologue), len(prologue), statics.data_ptr(),
                0 if statics.dim() == 1 else statics.stride(0), ephemerals.data_ptr(),
                payload.data_ptr() if plen else None, 0 if payload is None or payload.dim() == 1 else payload.stride(0),
                plen, n, msg1.data_ptr(), msg1.stride(0), lens.data_ptr(), states.data_ptr()))
            return out
        eph = np.ascontiguousarray(ephemerals, np.uint8).reshape(-1, 32)
        n = len(eph)
        st = np.frombuffer(bytes(statics), np.uint8) if isinstance(statics, (bytes, bytearray)) else \
            np.ascontiguousarray(statics, np.uint8).reshape(n, 32)
        one = isinstance(payload, (bytes, bytearray))
        pays = [bytes(payload)] if one else [bytes(p) for p in payload]
        plen = len(pays[0]) if pays else 0
        if any(len(p) != plen for p in pays) or (not one and len(pays) != n):
            raise ValueError("noise_ix_initiate: one payload length per call")
        pay = np.frombuffer(b"".join(pays), np.uint8) if plen else None
        stride = msg1_stride if msg1_stride is not None else 64 + plen
        msg1, lens, states = np.zeros((n, max(stride, 1)), np.uint8), np.zeros(n, np.uint32), np.zeros((n, 64), np.uint8)
        self._check(self.lib.gvs_noise_ix_initiate(
            self.h, cipher, bytes(prologue), len(prologue), st.ctypes.data, 0 if st.ndim == 1 else 32,
            eph.ctypes.data, pay.ctypes.data if pay is not None else None, 0 if one else plen, plen, n,
            msg1.ctypes.data, stride, lens.ctypes.data, states.ctypes.data))
        return [msg1[k, :lens[k]].tobytes() for k in range(n)], states, msg1

    def noise_ix_finish(self, statics, ephemerals, states, msg2, msg2_lens=None, payload2_stride=None, cipher=None,
                        device=False, out=None):
        """The initiator's reading of message 2 (gvs_noise_ix_finish; payload
        2 <= abi.AEAD_TEXT_MAX bytes): statics, ephemerals and cipher as in
        `noise_ix_initiate`, states what it returned, msg2 a list of n second
        messages -> (remote statics (n, 32), list of n payloads, send_keys
        (n, 32), recv_keys (n, 32), hashes (n, 64), (n,) bool, the (n, stride)
        payload slab).  A handshake that fails is all zero with b"".
        device=True is gvs_noise_ix_finish_device on torch CUDA tensors: msg2
        (n, stride >= 96) uint8 with msg2_lens (n,) int32; out =
        (remote_statics, payload2 (n, stride), payload2_lens, send_keys,
        recv_keys, hashes, ok) is written in place (made when None) and
        returned."""
        cipher = abi.CIPHER_AESGCM if cipher is None else cipher
        if device:
            import torch
            n = msg2.shape[0]
            if out is None:
                u8 = lambda w: torch.zeros((n, w), dtype=torch.uint8, device=msg2.device)
                i32 = lambda: torch.zeros(n, dtype=torch.int32, device=msg2.device)
                p2s = payload2_stride if payload2_stride is not None else max(msg2.stride(0) - 96, 1)
                out = (u8(32), u8(p2s), i32(), u8(32), u8(32), u8(64), i32())
            rs, pay, plens, sk, rk, hh, ok = out
            self._check(self.lib.gvs_noise_ix_finish_device(
                self.h, cipher, statics.data_ptr(), 0 if statics.dim() == 1 else statics.stride(0),
                ephemerals.data_ptr(), states.data_ptr(), msg2.data_ptr(), msg2.stride(0), msg2_lens.data_ptr(), n,
                rs.data_ptr(), pay.data_ptr(), pay.stride(0), plens.data_ptr(), sk.data_ptr(), rk.data_ptr(),
                hh.data_ptr() if hh is not None else None, ok.data_ptr()))
            return out
        eph = np.ascontiguousarray(ephemerals, np.uint8).reshape(-1, 32)
        n = len(eph)
        st = np.frombuffer(bytes(statics), np.uint8) if isinstance(statics, (bytes, bytearray)) else \
            np.ascontiguousarray(statics, np.uint8).reshape(n, 32)
        states = np.ascontiguousarray(states, np.uint8).reshape(n, 64)
        slab, lens, stride = self._wire_slab(msg2, max([len(m) for m in msg2] + [96]))
        p2s = payload2_stride if payload2_stride is not None else max(stride - 96, 1)
        pay, plens, ok = np.zeros((n, p2s), np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        rs, sk, rk, hh = (np.zeros((n, w), np.uint8) for w in (32, 32, 32, 64))
        self._check(self.lib.gvs_noise_ix_finish(
            self.h, cipher, st.ctypes.data, 0 if st.ndim == 1 else 32, eph.ctypes.data, states.ctypes.data,
            slab.ctypes.data, stride, lens.ctypes.data, n, rs.ctypes.data, pay.ctypes.data, p2s, plens.ctypes.data,
            sk.ctypes.data, rk.ctypes.data, hh.ctypes.data, ok.ctypes.data))
        return rs, [pay[k, :plens[k]].tobytes() for k in range(n)], sk, rk, hh, ok.astype(bool), pay

    def access(self, req):
        out = self.process_batch(np.asarray([req], dtype=abi.REQUEST_DTYPE) if not isinstance(req, np.ndarray) else req.reshape(1))
        return out[0]

    def stats(self):
        s = abi.GvsStats()
        self._check(self.lib.gvs_get_stats(self.h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in abi.GvsStats._fields_}

    def dump_messages(self):
        n = self.config.msg_capacity * self.stats()["shards"]
        out = np.zeros(n, dtype=abi.RECORD_DTYPE)
        self._check(self.lib.gvs_dump_messages(self.h, out.ctypes.data, n * 1024))
        return out

    def dump_raw_size(self, region, shard=0):
        """Size in bytes of one shard's raw region (abi.RAW_*).  Test use."""
        n = ctypes.c_uint64()
        self._check(self.lib.gvs_raw_size(self.h, shard, region, ctypes.byref(n)))
        return n.value

    def dump_raw(self, region, offset, nbytes, shard=0):
        """Raw device bytes of one shard's region (abi.RAW_*): ciphertext in
        authenticated mode.  Test use."""
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self.lib.gvs_dump_raw(self.h, shard, region, offset, out.ctypes.data, nbytes))
        return out

    def store_raw(self, region, offset, data, shard=0):
        """Overwrite raw device bytes (tamper tests of the authenticated mode)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        self._check(self.lib.gvs_store_raw(self.h, shard, region, offset, buf.ctypes.data, len(buf)))

    def synchronize(self):
        self._check(self.lib.gvs_synchronize(self.h))

    def set_option(self, key, value):
        self._check(self.lib.gvs_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = ctypes.c_int64()
        self._check(self.lib.gvs_get_option(self.h, key.encode(), ctypes.byref(v)))
        return v.value

    def set_expiry_cutoff(self, cutoff):
        """Messages with timestamp < cutoff expire (gvs_set_expiry_cutoff)."""
        self._check(self.lib.gvs_set_expiry_cutoff(self.h, int(cutoff)))

    def set_timing(self, on=True):
        self._check(self.lib.gvs_set_timing(self.h, 1 if on else 0))

    def last_timings(self):
        names = (ctypes.c_char_p * 32)()  # a channel wire batch has more than 16 stages
        ms = (ctypes.c_float * 32)()
        c = self.lib.gvs_last_timings(self.h, names, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(max(c, 0))}


class BlockStore:
    """The block store (gvs_oram_*): mc-oblivious-traits ORAM::access, batched.
    `access(ops)` applies abi.BLOCK_OP_DTYPE ops in order and returns the
    (n, 1024) blocks they saw."""

    def __init__(self, config):
        self.lib = load_library()
        self.config = config
        h = ctypes.c_void_p()
        rc = self.lib.gvs_oram_create(ctypes.byref(config), ctypes.byref(h))
        if rc != 0:
            raise GvsError(rc, "gvs_oram_create failed (no GPU, bad config or out of memory)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvs_oram_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise GvsError(rc, self.lib.gvs_oram_last_error(self.h).decode())

    def access(self, ops):
        ops = np.ascontiguousarray(ops, dtype=abi.BLOCK_OP_DTYPE)
        out = np.zeros((len(ops), 1024), dtype=np.uint8)
        self._check(self.lib.gvs_oram_access_batch(self.h, ops.ctypes.data, len(ops), out.ctypes.data))
        return out

    def access_device(self, d_ops, n, d_out):
        """Device pointers (ints): n ops in, n x 1024 bytes out."""
        self._check(self.lib.gvs_oram_access_batch_device(self.h, d_ops, n, d_out))

    def _raw_handle(self):
        if not hasattr(self.lib, "gvs_oram_test_handle"):
            raise RuntimeError("raw regions need the test library (GVS_TEST_HOOKS=1)")
        return self.lib.gvs_oram_test_handle(self.h)

    def dump_raw(self, region, offset, nbytes):
        """Raw device bytes of the block table (abi.RAW_MESSAGES), its tags
        (RAW_MSG_TAGS) or its pending final states (RAW_PENDING*).  Test use."""
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self.lib.gvs_dump_raw(self._raw_handle(), 0, region, offset, out.ctypes.data, nbytes))
        return out

    def store_raw(self, region, offset, data):
        """Overwrite raw device bytes (tamper tests of the sealed block store)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        self._check(self.lib.gvs_store_raw(self._raw_handle(), 0, region, offset, buf.ctypes.data, len(buf)))

    def set_timing(self, on=True):
        self._check(self.lib.gvs_oram_set_timing(self.h, 1 if on else 0))

    def last_timings(self):
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        c = self.lib.gvs_oram_last_timings(self.h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(max(c, 0))}


class KeyValueMap:
    """The key-value map (gvs_omap_*): mc-oblivious-traits ObliviousHashMap,
    batched.  `access(ops)` applies abi.OMAP_OP_DTYPE ops in order and returns
    abi.OMAP_RESULT_DTYPE results (status, the value each op saw)."""

    def __init__(self, config):
        self.lib = load_library()
        self.config = config
        h = ctypes.c_void_p()
        rc = self.lib.gvs_omap_create(ctypes.byref(config), ctypes.byref(h))
        if rc != 0:
            raise GvsError(rc, "gvs_omap_create failed (no GPU, bad config or out of memory)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvs_omap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise GvsError(rc, self.lib.gvs_omap_last_error(self.h).decode())

    def access(self, ops):
        ops = np.ascontiguousarray(ops, dtype=abi.OMAP_OP_DTYPE)
        out = np.zeros(len(ops), dtype=abi.OMAP_RESULT_DTYPE)
        self._check(self.lib.gvs_omap_access_batch(self.h, ops.ctypes.data, len(ops), out.ctypes.data))
        return out

    def access_device(self, d_ops, n, d_out):
        self._check(self.lib.gvs_omap_access_batch_device(self.h, d_ops, n, d_out))

    def _raw_handle(self):
        if not hasattr(self.lib, "gvs_omap_test_handle"):
            raise RuntimeError("raw regions need the test library (GVS_TEST_HOOKS=1)")
        return self.lib.gvs_omap_test_handle(self.h)

    def dump_raw(self, region, offset, nbytes):
        """Raw device bytes of the value table and its regions (as BlockStore),
        the key directory (abi.RAW_KEY_DIR) or its tags (RAW_KEY_DIR_TAGS)."""
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self.lib.gvs_dump_raw(self._raw_handle(), 0, region, offset, out.ctypes.data, nbytes))
        return out

    def store_raw(self, region, offset, data):
        """Overwrite raw device bytes (tamper tests of the sealed map)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        self._check(self.lib.gvs_store_raw(self._raw_handle(), 0, region, offset, buf.ctypes.data, len(buf)))

    def set_timing(self, on=True):
        self._check(self.lib.gvs_omap_set_timing(self.h, 1 if on else 0))

    def last_timings(self):
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        c = self.lib.gvs_omap_last_timings(self.h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(max(c, 0))}
