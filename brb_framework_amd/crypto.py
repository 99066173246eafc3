"""ctypes binding of libbrb_crypto_gpu.so (include/brb_crypto.h).  Test/bench plumbing only."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# BRB_CRYPTO_LIB: another build of the same library for the test plumbing (the ASan/UBSan build of
# tools/sanitize_check.sh); the C library itself reads no environment variable.
LIB_PATH = os.environ.get("BRB_CRYPTO_LIB") or os.path.join(HERE, "libbrb_crypto_gpu.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "brb_crypto.h")

BATCH_HOST = 0x0
BATCH_DEVICE = 0x1
BATCH_ASYNC = 0x2
BATCH_ALL_DEVICES = 0x4
BATCH_DROPPED = -2
BATCH_PARTIAL = -3
BATCH_FAULT = -4
TRANSFORM_DROPPED = -1

u8p = ctypes.POINTER(ctypes.c_uint8)
ulp = ctypes.POINTER(ctypes.c_ulong)


class BRB_MD5_CTX(ctypes.Structure):
    """libbrb_data.h:854-860"""
    _fields_ = [("buf", ctypes.c_uint32 * 4), ("bytes", ctypes.c_uint32 * 2), ("in_", ctypes.c_uint32 * 16),
                ("digest", ctypes.c_ubyte * 16), ("string", ctypes.c_ubyte * 64)]


class BrbSha1Ctx(ctypes.Structure):
    """libbrb_data.h:1937-1943"""
    _fields_ = [("state", ctypes.c_uint32 * 5), ("count", ctypes.c_uint32 * 2), ("buffer", ctypes.c_uint8 * 64)]


class BRB_BLOWFISH_CTX(ctypes.Structure):
    """libbrb_data.h:876-879 (LP64: unsigned long = 8 bytes)"""
    _fields_ = [("P", ctypes.c_ulong * 18), ("S", (ctypes.c_ulong * 256) * 4)]


class _Rc4Flags(ctypes.Structure):
    _fields_ = [("initialized", ctypes.c_uint, 1)]


class BRB_RC4_State(ctypes.Structure):
    """libbrb_data.h:887-897"""
    _fields_ = [("perm", ctypes.c_ubyte * 256), ("index1", ctypes.c_ubyte), ("index2", ctypes.c_ubyte),
                ("flags", _Rc4Flags)]


assert ctypes.sizeof(BRB_MD5_CTX) == 168 and ctypes.sizeof(BrbSha1Ctx) == 92
assert ctypes.sizeof(BRB_BLOWFISH_CTX) == 8336 and ctypes.sizeof(BRB_RC4_State) == 264
RC4_STATE_BYTES = 264
RC4MD5_HEADER = 30

_LIB = None

# (name, restype, argtypes) of every function include/brb_crypto.h declares
_SIGNATURES = [
    ("BRB_MD5Init", None, [ctypes.POINTER(BRB_MD5_CTX)]),
    ("BRB_MD5UpdateBig", None, [ctypes.POINTER(BRB_MD5_CTX), ctypes.c_void_p, ctypes.c_ulong]),
    ("BRB_MD5Update", None, [ctypes.POINTER(BRB_MD5_CTX), ctypes.c_void_p, ctypes.c_ulong]),
    ("BRB_MD5UpdateLowerText", None, [ctypes.POINTER(BRB_MD5_CTX), ctypes.c_char_p, ctypes.c_int]),
    ("BRB_MD5Final", None, [ctypes.POINTER(BRB_MD5_CTX)]),
    ("BRB_MD5Transform", None, [ctypes.POINTER(BRB_MD5_CTX)]),
    ("BRB_MD5LateInitDigestString", None, [ctypes.POINTER(BRB_MD5_CTX)]),
    ("BRB_MD5ToStr", None, [ctypes.c_void_p, ctypes.c_void_p]),
    ("BrbSha1_Init", None, [ctypes.POINTER(BrbSha1Ctx)]),
    ("BrbSha1_Update", None, [ctypes.POINTER(BrbSha1Ctx), ctypes.c_void_p, ctypes.c_size_t]),
    ("BrbSha1_Final", None, [ctypes.POINTER(BrbSha1Ctx), ctypes.c_void_p]),
    ("BrbSha1_Transform", None, [ctypes.c_void_p, ctypes.c_void_p]),
    ("BrbSha1_Do", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    ("BRB_Blowfish_Init", None, [ctypes.POINTER(BRB_BLOWFISH_CTX), ctypes.c_void_p, ctypes.c_int]),
    ("BRB_Blowfish_Encrypt", None, [ctypes.POINTER(BRB_BLOWFISH_CTX), ulp, ulp]),
    ("BRB_Blowfish_Decrypt", None, [ctypes.POINTER(BRB_BLOWFISH_CTX), ulp, ulp]),
    ("BRB_RC4_Init", None, [ctypes.POINTER(BRB_RC4_State), ctypes.c_void_p, ctypes.c_int]),
    ("BRB_RC4_Crypt", None, [ctypes.POINTER(BRB_RC4_State), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("BRB_MD5BatchFixed", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MD5Batch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MD5BatchSegments", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
      ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MetaDataUnpackBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MetaDataUnpackItemsBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MetaDataPackBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BrbSha1_BatchFixed", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BrbSha1_Batch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MD5InitBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MD5UpdateBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MD5FinalBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BrbSha1_InitBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BrbSha1_UpdateBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BrbSha1_FinalBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MD5UpdateSegmentsBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BrbSha1_UpdateSegmentsBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MD5LowerTextBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MD5UpdateSegmentsLowerBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_Blowfish_EncryptBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_Blowfish_DecryptBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_Blowfish_EncryptBatchKeyed", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_Blowfish_DecryptBatchKeyed", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MemBufferEncryptBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MemBufferDecryptBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4_InitBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_Blowfish_InitBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_TransformBatcherEnableBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("BRB_RC4_CryptBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
      ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4MD5_FrameBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4MD5_OpenBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
      ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4_CryptListBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4MD5_FrameListBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4MD5_OpenListBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_RC4_MixedListBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
      ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_Base64EncodeBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_Base64DecodeBatch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MemBufferKey", None, [ctypes.c_uint, ctypes.c_void_p]),
    ("BRB_MemBufferEncrypt", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_uint, ctypes.c_ulong, ctypes.POINTER(ctypes.c_ulong), ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_MemBufferDecrypt", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_uint, ctypes.c_ulong, ctypes.POINTER(ctypes.c_ulong), ctypes.c_uint,
      ctypes.c_void_p]),
    ("BRB_TransformBatcherCreate", ctypes.c_void_p, [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int]),
    ("BRB_TransformBatcherDestroy", None, [ctypes.c_void_p]),
    ("BRB_TransformBatcherEnable", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]),
    ("BRB_TransformBatcherEnableAlgo", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    ("BRB_TransformBatcherEnableBatchAlgo", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("BRB_TransformBatcherDisable", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    ("BRB_TransformBatcherRead", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]),
    ("BRB_TransformBatcherWrite", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]),
    ("BRB_TransformBatcherFlush", ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("BRB_TransformBatcherFlushAsync", ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("BRB_TransformBatcherGetState", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(BRB_RC4_State)]),
    ("BRB_TransformBatcherInjectFault", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("BRB_CryptoGPU_TestOption", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("BRB_CryptoGPU_TestFixedRoute", ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint32]),
    ("BRB_CryptoGPU_HostRegister", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    ("BRB_CryptoGPU_HostUnregister", ctypes.c_int, [ctypes.c_void_p]),
    ("BRB_CryptoGPU_Available", ctypes.c_int, []),
    ("BRB_CryptoGPU_DeviceCount", ctypes.c_int, []),
    ("BRB_CryptoGPU_SetDevice", ctypes.c_int, [ctypes.c_int]),
    ("BRB_CryptoGPU_GetDevice", ctypes.c_int, []),
    ("BRB_CryptoGPU_ThreadCleanup", None, []),
    ("BRB_CryptoGPU_LastError", ctypes.c_char_p, []),
    ("BRB_CryptoGPU_AsyncFaultCheck", ctypes.c_int, []),
    ("BRB_CryptoGPU_Version", ctypes.c_char_p, []),
]


def lib() -> ctypes.CDLL:
    """Load the in-tree library; raise if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {HERE}` "
                               "(or __graft_entry__.build())")
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 and
        # libhsa-runtime64.so.1.  Loading torch first lets the dynamic loader resolve this
        # library's DT_NEEDED libamdhip64.so.7 to that same copy (glibc matches by SONAME);
        # the other order maps two HSA runtimes and the second sees no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in _SIGNATURES:
            f = getattr(L, name, None)
            if f is None:
                # An older build (interleaved A/B runs load one): the library still loads, but the
                # first call of a symbol it lacks raises here, naming it, instead of failing later
                # with default ctypes argtypes.  tests/test_abi.py checks exports == header.
                setattr(L, name, _missing_symbol(name))
                continue
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _missing_symbol(name: str):
    def call(*_a, **_k):
        raise RuntimeError(f"{LIB_PATH} does not export {name} (a stale build?): rebuild with `make -C {HERE}`")
    return call


def exported_symbols() -> set:
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def gpu_available() -> bool:
    return bool(lib().BRB_CryptoGPU_Available())


def async_fault_check() -> None:
    """BRB_CryptoGPU_AsyncFaultCheck: raises (returned -4) if a wave-pair kernel of this thread's
    async device-mode calls reported a protocol fault since the last check.  Synchronise first."""
    _check(lib().BRB_CryptoGPU_AsyncFaultCheck(), "BRB_CryptoGPU_AsyncFaultCheck")


def test_option(name: str, value: int) -> int:
    """BRB_CryptoGPU_TestOption: sets a process-wide A/B switch, returns its previous value."""
    old = ctypes.c_int(0)
    _check(lib().BRB_CryptoGPU_TestOption(name.encode(), int(value), ctypes.byref(old)), "BRB_CryptoGPU_TestOption")
    return old.value


class TestOption:
    """Context manager: `with TestOption("var_line", 0): ...` restores the previous value on exit."""

    __test__ = False     # not a pytest class

    def __init__(self, name: str, value: int):
        self.name, self.value, self.old = name, value, None

    def __enter__(self):
        self.old = test_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        test_option(self.name, self.old)
        return False


# BRB_FIXED_ROUTE_* (include/brb_crypto.h), in launch order
(FIXED_ROUTE_LANE_A4, FIXED_ROUTE_LANE_ANY, FIXED_ROUTE_LINE, FIXED_ROUTE_VAR_LINE, FIXED_ROUTE_DMA_TICKET,
 FIXED_ROUTE_B64R_8, FIXED_ROUTE_B64R_4, FIXED_ROUTE_B64, FIXED_ROUTE_DMA_SHORT) = range(9)


def fixed_route(addr: int, rec_len: int) -> int:
    """BRB_CryptoGPU_TestFixedRoute: the FIXED_ROUTE_* kernel choice of a fixed-stride digest call for
    records of rec_len bytes at address addr, under the current test options (no device needed)."""
    return lib().BRB_CryptoGPU_TestFixedRoute(int(addr), int(rec_len))


def _check(rc: int, what: str) -> None:
    if rc != 1:
        msg = lib().BRB_CryptoGPU_LastError().decode(errors="replace")
        raise RuntimeError(f"{what} returned {rc}: {msg}")


# ---- buffer helpers ---------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(x) -> int:
    if x is None:
        return 0
    if _is_torch(x):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data
    raise TypeError(f"unsupported buffer type {type(x)}")


def _mode(data, stream, async_, all_devices=False):
    """(flags, stream_handle) for a buffer: torch CUDA tensor -> device mode, numpy -> host mode
    (all_devices: BRB_BATCH_ALL_DEVICES, host mode only)."""
    if all_devices:
        if _is_torch(data):
            raise ValueError("all_devices needs host (numpy) buffers")
        return BATCH_HOST | BATCH_ALL_DEVICES, 0
    if _is_torch(data):
        if not data.is_cuda:
            raise ValueError("torch tensors must live on a CUDA (HIP) device; pass numpy for host mode")
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(data.device)
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        return BATCH_DEVICE | (BATCH_ASYNC if async_ else 0), handle
    return BATCH_HOST, (int(stream) if stream is not None else 0)


def _out_like(data, n, width):
    if _is_torch(data):
        import torch
        return torch.empty((n, width), dtype=torch.uint8, device=data.device)
    return np.empty((n, width), dtype=np.uint8)


def _nbytes(x) -> int:
    return x.numel() * x.element_size() if _is_torch(x) else x.nbytes


def _digest_fixed(fn, width, data, rec_len, n, out, stream, async_, all_devices=False):
    if n is None:
        n = _nbytes(data) // rec_len if rec_len else 0
    if rec_len * n > _nbytes(data):
        raise ValueError("data is smaller than rec_len * n")
    if out is None:
        out = _out_like(data, n, width)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(fn(_ptr(data), rec_len, n, _ptr(out), flags, h), fn.__name__)
    return out


def _digest_var(fn, width, data, offsets, lengths, out, stream, async_, all_devices=False):
    n = len(offsets)
    if out is None:
        out = _out_like(data, n, width)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(fn(_ptr(data), _ptr(offsets), _ptr(lengths), n, _ptr(out), flags, h), fn.__name__)
    return out


def md5_batch_fixed(data, rec_len, n=None, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5BatchFixed: digests (n, 16) of n records of rec_len bytes stored back to back."""
    return _digest_fixed(lib().BRB_MD5BatchFixed, 16, data, rec_len, n, out, stream, async_, all_devices)


def sha1_batch_fixed(data, rec_len, n=None, out=None, stream=None, async_=False, all_devices=False):
    """BrbSha1_BatchFixed: digests (n, 20)."""
    return _digest_fixed(lib().BrbSha1_BatchFixed, 20, data, rec_len, n, out, stream, async_, all_devices)


def md5_batch(data, offsets, lengths, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5Batch: offsets uint64[n], lengths uint32[n] (same memory kind as data)."""
    return _digest_var(lib().BRB_MD5Batch, 16, data, offsets, lengths, out, stream, async_, all_devices)


def md5_lower_text_batch(data, offsets, lengths, out=None, strings=None, want_strings=False, stream=None, async_=False,
                          all_devices=False):
    """BRB_MD5LowerTextBatch: the MD5 of key i = data[offsets[i]:+lengths[i]] lower-cased as BRB_MD5UpdateLowerText
    does ('A'..'Z' only), without a context.  Returns the digests (n, 16); with `strings` given or want_strings,
    (digests, strings), strings (n, 33) uint8 holding 32 lower-case hex characters and a NUL per key."""
    _same_kind(data, offsets, lengths, out, strings)
    n = len(offsets)
    if len(lengths) != n:
        raise ValueError("offsets and lengths differ in length")
    if out is None:
        out = _out_like(data, n, 16)
    elif _nbytes(out) < n * 16:
        raise ValueError(f"out holds {_nbytes(out)} bytes, {n} digests need {n * 16}")
    if strings is None and want_strings:
        strings = _out_like(data, n, 33)
    elif strings is not None and _nbytes(strings) < n * 33:
        raise ValueError(f"strings holds {_nbytes(strings)} bytes, {n} keys need {n * 33}")
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_MD5LowerTextBatch(_ptr(data), _ptr(offsets), _ptr(lengths), n, _ptr(out), _ptr(strings), flags, h),
           "BRB_MD5LowerTextBatch")
    return out if strings is None else (out, strings)


def md5_batch_segments(data, seg_offsets, seg_lengths, rec_first_seg, out=None, stream=None, async_=False,
                       all_devices=False):
    """BRB_MD5BatchSegments: record i = concatenation of segments rec_first_seg[i] .. rec_first_seg[i+1]-1
    (the MetaData pack digest).  rec_first_seg has n + 1 entries."""
    n = len(rec_first_seg) - 1
    if out is None:
        out = _out_like(data, n, 16)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_MD5BatchSegments(_ptr(data), _ptr(seg_offsets), _ptr(seg_lengths), _ptr(rec_first_seg), n,
                                      _ptr(out), flags, h), "BRB_MD5BatchSegments")
    return out


# BRB_MetaDataUnpackInfo (include/brb_crypto.h), one per pack
METADATA_INFO_DTYPE = np.dtype([("error_code", "<i4"), ("item_count", "<u4"), ("cur_offset", "<u8"),
                                ("cur_remaining", "<u8"), ("cur_needed", "<u8")])


def metadata_unpack_batch(data, offsets, lengths, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MetaDataUnpackBatch: MetaDataUnpack (meta_data.c:145-328) of pack i = data[offsets[i] ..
    + lengths[i]); returns one BRB_MetaDataUnpackInfo per pack (numpy structured array in host mode,
    an (n, 32) uint8 tensor in device mode)."""
    n = len(offsets)
    if out is None:
        if _is_torch(data):
            import torch
            out = torch.empty((n, METADATA_INFO_DTYPE.itemsize), dtype=torch.uint8, device=data.device)
        else:
            out = np.empty(n, METADATA_INFO_DTYPE)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_MetaDataUnpackBatch(_ptr(data), _ptr(offsets), _ptr(lengths), n, _ptr(out), flags, h),
           "BRB_MetaDataUnpackBatch")
    return out


def metadata_unpack_items_batch(data, offsets, lengths, item_offsets, item_lengths, item_ids, item_sub_ids,
                                pack_first_slot, items_added=None, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MetaDataUnpackItemsBatch: metadata_unpack_batch plus the item table.  Pack p's j-th MetaDataItemAdd
    call (j below pack_first_slot[p + 1] - pack_first_slot[p]; n + 1 entries) is written to slot
    pack_first_slot[p] + j of item_offsets (uint64: the data's offset in `data`), item_lengths (uint32),
    item_ids and item_sub_ids (uint64); other slots keep their values.  numpy arrays in host mode, CUDA tensors
    (int64 / int32) in device mode, all of one kind.  Returns (info, items_added): info as metadata_unpack_batch
    returns it, items_added uint32[n] (an int32 tensor in device mode) = calls per pack, stored or not."""
    _same_kind(data, offsets, lengths, item_offsets, item_lengths, item_ids, item_sub_ids, pack_first_slot, items_added,
               out)
    n = len(offsets)
    if len(lengths) != n or len(pack_first_slot) != n + 1:
        raise ValueError("lengths needs n entries and pack_first_slot n + 1")
    if not (len(item_offsets) == len(item_lengths) == len(item_ids) == len(item_sub_ids)):
        raise ValueError("the four item arrays differ in length")
    if _is_torch(data):
        import torch
        if out is None:
            out = torch.empty((n, METADATA_INFO_DTYPE.itemsize), dtype=torch.uint8, device=data.device)
        if items_added is None:
            items_added = torch.empty(n, dtype=torch.int32, device=data.device)
    else:
        if out is None:
            out = np.empty(n, METADATA_INFO_DTYPE)
        if items_added is None:
            items_added = np.empty(n, np.uint32)
        if n and int(pack_first_slot[n]) > len(item_offsets):
            raise ValueError("pack_first_slot ends past the item arrays")
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_MetaDataUnpackItemsBatch(_ptr(data), _ptr(offsets), _ptr(lengths), n, _ptr(out), _ptr(item_offsets),
                                              _ptr(item_lengths), _ptr(item_ids), _ptr(item_sub_ids),
                                              _ptr(pack_first_slot), _ptr(items_added), flags, h),
           "BRB_MetaDataUnpackItemsBatch")
    return out, items_added


def metadata_pack_batch(data, item_offsets, item_lengths, item_ids, item_sub_ids, pack_first_item, out, out_offsets,
                        stream=None, async_=False, all_devices=False):
    """BRB_MetaDataPackBatch: MetaDataPack (meta_data.c:104-140) of pack p = items pack_first_item[p] ..
    pack_first_item[p + 1] - 1 (n + 1 entries), item k = data[item_offsets[k] .. + item_lengths[k]) with
    item_ids[k], item_sub_ids[k], written at out[out_offsets[p]:].  numpy arrays in host mode, CUDA
    tensors in device mode (all nine the same kind); returns out."""
    _same_kind(data, item_offsets, item_lengths, item_ids, item_sub_ids, pack_first_item, out, out_offsets)
    n = len(pack_first_item) - 1
    if n < 0 or len(out_offsets) < n:
        raise ValueError("pack_first_item needs n + 1 entries and out_offsets n")
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_MetaDataPackBatch(_ptr(data), _ptr(item_offsets), _ptr(item_lengths), _ptr(item_ids),
                                       _ptr(item_sub_ids), _ptr(pack_first_item), n, _ptr(out), _ptr(out_offsets),
                                       flags, h), "BRB_MetaDataPackBatch")
    return out


def sha1_batch(data, offsets, lengths, out=None, stream=None, async_=False, all_devices=False):
    return _digest_var(lib().BrbSha1_Batch, 20, data, offsets, lengths, out, stream, async_, all_devices)


# ---- streaming MD5 / SHA-1 contexts as a batch ----------------------------------------------------
MD5_CTX_BYTES = 168
SHA1_CTX_BYTES = 92


def _ctx_row(row, ctype):
    """A pointer to the compat struct held in one row of a host context table."""
    if not (isinstance(row, np.ndarray) and row.dtype == np.uint8 and row.flags["C_CONTIGUOUS"]
            and row.nbytes == ctypes.sizeof(ctype)):
        raise ValueError(f"a context row is a contiguous uint8 array of {ctypes.sizeof(ctype)} bytes")
    return ctypes.cast(row.ctypes.data, ctypes.POINTER(ctype))


def md5_ctx_init(row) -> None:
    """BRB_MD5Init (host, compat) on one row of a (n_ctx, 168) table."""
    lib().BRB_MD5Init(_ctx_row(row, BRB_MD5_CTX))


def md5_ctx_update(row, piece) -> None:
    """BRB_MD5Update (host, compat) of one row with `piece` (bytes)."""
    piece = bytes(piece)
    lib().BRB_MD5Update(_ctx_row(row, BRB_MD5_CTX), ctypes.create_string_buffer(piece, max(len(piece), 1)), len(piece))


def md5_ctx_update_lower(row, piece) -> None:
    """BRB_MD5UpdateLowerText (host, compat) of one row with `piece` (bytes): 'A'..'Z' lower-cased on the way in."""
    piece = bytes(piece)
    lib().BRB_MD5UpdateLowerText(_ctx_row(row, BRB_MD5_CTX), ctypes.create_string_buffer(piece, max(len(piece), 1)),
                                 len(piece))


def md5_ctx_final(row) -> bytes:
    """BRB_MD5Final (host, compat) of one row; returns the 16 digest bytes."""
    lib().BRB_MD5Final(_ctx_row(row, BRB_MD5_CTX))
    return row[88:104].tobytes()


def sha1_ctx_init(row) -> None:
    """BrbSha1_Init (host, compat) on one row of a (n_ctx, 92) table."""
    lib().BrbSha1_Init(_ctx_row(row, BrbSha1Ctx))


def sha1_ctx_update(row, piece) -> None:
    """BrbSha1_Update (host, compat) of one row with a private copy of `piece` (the call rewrites its input)."""
    piece = bytes(piece)
    lib().BrbSha1_Update(_ctx_row(row, BrbSha1Ctx), ctypes.create_string_buffer(piece, max(len(piece), 1)), len(piece))


def sha1_ctx_final(row) -> bytes:
    """BrbSha1_Final (host, compat) of one row (zeroed afterwards); returns the 20 digest bytes."""
    out = ctypes.create_string_buffer(20)
    lib().BrbSha1_Final(_ctx_row(row, BrbSha1Ctx), out)
    return out.raw


def _stream_n(ctxs, width, ctx_index, n):
    """(n_ctx, n) of a context-table call: n defaults to len(ctx_index), or to the whole table."""
    if _nbytes(ctxs) % width:
        raise ValueError(f"ctxs holds {_nbytes(ctxs)} bytes, not a multiple of {width}")
    n_ctx = _nbytes(ctxs) // width
    if ctx_index is not None:
        if n is not None and n != len(ctx_index):
            raise ValueError("n differs from len(ctx_index)")
        return n_ctx, len(ctx_index)
    return n_ctx, n_ctx if n is None else n


def _stream_init(fn, width, ctxs, ctx_index, n, stream, async_, all_devices):
    _same_kind(ctxs, ctx_index)
    n_ctx, n = _stream_n(ctxs, width, ctx_index, n)
    flags, h = _mode(ctxs, stream, async_, all_devices)
    _check(fn(_ptr(ctxs), n_ctx, _ptr(ctx_index), n, flags, h), fn.__name__)
    return ctxs


def _stream_update(fn, width, ctxs, data, offsets, lengths, ctx_index, stream, async_, all_devices):
    _same_kind(ctxs, data, offsets, lengths, ctx_index)
    n_ctx, n = _stream_n(ctxs, width, ctx_index, len(offsets))
    if len(lengths) != n:
        raise ValueError("offsets, lengths and ctx_index differ in length")
    flags, h = _mode(ctxs, stream, async_, all_devices)
    _check(fn(_ptr(ctxs), n_ctx, _ptr(ctx_index), _ptr(data), _ptr(offsets), _ptr(lengths), n, flags, h), fn.__name__)
    return ctxs


def _stream_final(fn, width, dig, ctxs, ctx_index, n, out, stream, async_, all_devices):
    _same_kind(ctxs, ctx_index, out)
    n_ctx, n = _stream_n(ctxs, width, ctx_index, n)
    if out is None:
        out = _out_like(ctxs, n, dig)
    elif _nbytes(out) < n * dig:
        raise ValueError(f"out holds {_nbytes(out)} bytes, {n} digests need {n * dig}")
    flags, h = _mode(ctxs, stream, async_, all_devices)
    _check(fn(_ptr(ctxs), n_ctx, _ptr(ctx_index), n, _ptr(out), flags, h), fn.__name__)
    return out


def _stream_segments(fn, width, dig, ctxs, data, seg_offsets, seg_lengths, item_first_seg, final, ctx_index, out, stream,
                     async_, all_devices, seg_lower=False):
    """seg_lower: False for the calls without the list; else BRB_MD5UpdateSegmentsLowerBatch's (None: NULL)."""
    if seg_lower is False:
        seg_lower, lower = None, ()
    else:
        lower = (_ptr(seg_lower),)
    if seg_lower is not None and (len(seg_lower) != len(seg_lengths) or _nbytes(seg_lower) != len(seg_lengths)):
        raise ValueError("seg_lower is one byte per segment")
    _same_kind(ctxs, data, seg_offsets, seg_lengths, item_first_seg, final, ctx_index, out, seg_lower)
    n_ctx, n = _stream_n(ctxs, width, ctx_index, len(item_first_seg) - 1)
    if n < 0 or len(seg_offsets) != len(seg_lengths):
        raise ValueError("item_first_seg needs n + 1 entries, and seg_offsets as many as seg_lengths")
    if final is None:
        out = None
    else:
        if len(final) != n or _nbytes(final) != n:
            raise ValueError("final is one byte per item")
        if out is None:
            out = _out_like(ctxs, n, dig)
            out[...] = 0                             # the rows of items that are not finalised are not written
        elif _nbytes(out) < n * dig:
            raise ValueError(f"out holds {_nbytes(out)} bytes, {n} digests need {n * dig}")
    flags, h = _mode(ctxs, stream, async_, all_devices)
    _check(fn(_ptr(ctxs), n_ctx, _ptr(ctx_index), _ptr(data), _ptr(seg_offsets), _ptr(seg_lengths), *lower,
              _ptr(item_first_seg), n, _ptr(final), _ptr(out), flags, h), fn.__name__)
    return out


def md5_update_segments_batch(ctxs, data, seg_offsets, seg_lengths, item_first_seg, final=None, ctx_index=None, out=None,
                              stream=None, async_=False, all_devices=False):
    """BRB_MD5UpdateSegmentsBatch: context ctx_index[i] (None: i) takes the segments item_first_seg[i] ..
    item_first_seg[i+1]-1 (n + 1 entries; segment k = data[seg_offsets[k]:+seg_lengths[k]]) in order, as one
    BRB_MD5UpdateBig each, and is then finalised when final[i] != 0 (final: uint8[n], None: no item).  Returns
    the digests (n, 16) -- only the rows of finalised items are written, the rest of a fresh `out` is 0 -- or
    None when final is None."""
    return _stream_segments(lib().BRB_MD5UpdateSegmentsBatch, MD5_CTX_BYTES, 16, ctxs, data, seg_offsets, seg_lengths,
                            item_first_seg, final, ctx_index, out, stream, async_, all_devices)


def md5_update_segments_lower_batch(ctxs, data, seg_offsets, seg_lengths, item_first_seg, seg_lower=None, final=None,
                                    ctx_index=None, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5UpdateSegmentsLowerBatch: md5_update_segments_batch with seg_lower, uint8 per segment -- != 0 takes the
    segment as BRB_MD5UpdateLowerText, 0 as BRB_MD5UpdateBig; None: every segment is lower-cased."""
    return _stream_segments(lib().BRB_MD5UpdateSegmentsLowerBatch, MD5_CTX_BYTES, 16, ctxs, data, seg_offsets, seg_lengths,
                            item_first_seg, final, ctx_index, out, stream, async_, all_devices, seg_lower=seg_lower)


def sha1_update_segments_batch(ctxs, data, seg_offsets, seg_lengths, item_first_seg, final=None, ctx_index=None, out=None,
                               stream=None, async_=False, all_devices=False):
    """BrbSha1_UpdateSegmentsBatch (see md5_update_segments_batch): digests (n, 20); a finalised context is zeroed."""
    return _stream_segments(lib().BrbSha1_UpdateSegmentsBatch, SHA1_CTX_BYTES, 20, ctxs, data, seg_offsets, seg_lengths,
                            item_first_seg, final, ctx_index, out, stream, async_, all_devices)


def md5_init_batch(ctxs, ctx_index=None, n=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5InitBatch: BRB_MD5Init of ctxs[ctx_index[i]] (ctx_index None: the first n contexts, all by
    default).  ctxs: (n_ctx, 168) uint8, numpy for host mode or a CUDA tensor for device mode (ctx_index
    uint32[n] / an int32 tensor of the same kind); updated in place and returned."""
    return _stream_init(lib().BRB_MD5InitBatch, MD5_CTX_BYTES, ctxs, ctx_index, n, stream, async_, all_devices)


def md5_update_batch(ctxs, data, offsets, lengths, ctx_index=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5UpdateBatch: context ctx_index[i] (None: i) takes the piece data[offsets[i]:+lengths[i]], as
    BRB_MD5Update would.  A context may be named once per call.  offsets uint64[n], lengths uint32[n]."""
    return _stream_update(lib().BRB_MD5UpdateBatch, MD5_CTX_BYTES, ctxs, data, offsets, lengths, ctx_index, stream,
                          async_, all_devices)


def md5_final_batch(ctxs, ctx_index=None, n=None, out=None, stream=None, async_=False, all_devices=False):
    """BRB_MD5FinalBatch: BRB_MD5Final of the named contexts (buf, digest, hex string); returns the
    digests (n, 16) in item order."""
    return _stream_final(lib().BRB_MD5FinalBatch, MD5_CTX_BYTES, 16, ctxs, ctx_index, n, out, stream, async_,
                         all_devices)


def sha1_init_batch(ctxs, ctx_index=None, n=None, stream=None, async_=False, all_devices=False):
    """BrbSha1_InitBatch (see md5_init_batch); ctxs: (n_ctx, 92) uint8."""
    return _stream_init(lib().BrbSha1_InitBatch, SHA1_CTX_BYTES, ctxs, ctx_index, n, stream, async_, all_devices)


def sha1_update_batch(ctxs, data, offsets, lengths, ctx_index=None, stream=None, async_=False, all_devices=False):
    """BrbSha1_UpdateBatch (see md5_update_batch); never writes into data."""
    return _stream_update(lib().BrbSha1_UpdateBatch, SHA1_CTX_BYTES, ctxs, data, offsets, lengths, ctx_index, stream,
                          async_, all_devices)


def sha1_final_batch(ctxs, ctx_index=None, n=None, out=None, stream=None, async_=False, all_devices=False):
    """BrbSha1_FinalBatch: returns the digests (n, 20); the named contexts are zeroed."""
    return _stream_final(lib().BrbSha1_FinalBatch, SHA1_CTX_BYTES, 20, ctxs, ctx_index, n, out, stream, async_,
                         all_devices)


# ---- Blowfish ------------------------------------------------------------------------------------
def blowfish_init(key: bytes, key_len: int | None = None) -> BRB_BLOWFISH_CTX:
    ctx = BRB_BLOWFISH_CTX()
    kb = ctypes.create_string_buffer(bytes(key), max(len(key), 1))
    lib().BRB_Blowfish_Init(ctypes.byref(ctx), kb, len(key) if key_len is None else key_len)
    return ctx


def blowfish_ctx_bytes(ctx: BRB_BLOWFISH_CTX) -> bytes:
    return ctypes.string_at(ctypes.addressof(ctx), ctypes.sizeof(ctx))


def _bf(fn, ctx, words, n_blocks, stream, async_, all_devices=False):
    """words: uint64 numpy array (host) or int64/uint64 torch CUDA tensor (device), 2 words per block.
    ctx: BRB_BLOWFISH_CTX (host mode) or, in device mode, a CUDA uint8 tensor holding its 8336 bytes
    (a BRB_BLOWFISH_CTX is uploaded for you)."""
    if n_blocks is None:
        n_blocks = _nbytes(words) // 16
    if 16 * n_blocks > _nbytes(words):
        raise ValueError("words holds fewer than n_blocks (xl, xr) pairs")
    flags, h = _mode(words, stream, async_, all_devices)
    if flags & BATCH_DEVICE:
        if isinstance(ctx, BRB_BLOWFISH_CTX):
            import torch
            ctx = torch.frombuffer(bytearray(blowfish_ctx_bytes(ctx)), dtype=torch.uint8).to(words.device)
        cptr = _ptr(ctx)
    else:
        cptr = ctypes.addressof(ctx)
    _check(fn(cptr, _ptr(words), n_blocks, flags, h), fn.__name__)
    return words


def blowfish_encrypt_batch(ctx, words, n_blocks=None, stream=None, async_=False, all_devices=False):
    return _bf(lib().BRB_Blowfish_EncryptBatch, ctx, words, n_blocks, stream, async_, all_devices)


def blowfish_decrypt_batch(ctx, words, n_blocks=None, stream=None, async_=False, all_devices=False):
    return _bf(lib().BRB_Blowfish_DecryptBatch, ctx, words, n_blocks, stream, async_, all_devices)


def blowfish_contexts(ctxs) -> np.ndarray:
    """A list of BRB_BLOWFISH_CTX -> the (n, 8336) uint8 array the keyed calls take as `ctxs`."""
    return np.frombuffer(b"".join(blowfish_ctx_bytes(c) for c in ctxs), np.uint8).reshape(len(ctxs), BLOWFISH_CTX_BYTES).copy()


def _bf_keyed(fn, ctxs, words, word_offsets, block_counts, ctx_index, stream, async_, all_devices):
    """words: uint64 numpy array (host) or int64/uint64 CUDA tensor (device); word_offsets uint64[n] (in 8-byte
    words), block_counts uint32[n], ctx_index uint32[n] or None, of the same kind.  ctxs: (n_ctx, 8336) uint8
    of that kind too (a blowfish_init_batch result as it stands), or a list of BRB_BLOWFISH_CTX / a numpy
    array, which device mode uploads for you."""
    if isinstance(ctxs, (list, tuple)):
        ctxs = blowfish_contexts(ctxs)
    flags, h = _mode(words, stream, async_, all_devices)
    if (flags & BATCH_DEVICE) and not _is_torch(ctxs):
        import torch
        ctxs = torch.from_numpy(np.ascontiguousarray(ctxs)).to(words.device)
    _same_kind(words, ctxs, word_offsets, block_counts, ctx_index)
    n = len(word_offsets)
    if len(block_counts) != n or (ctx_index is not None and len(ctx_index) != n):
        raise ValueError("word_offsets, block_counts and ctx_index differ in length")
    _check(fn(_ptr(ctxs), _nbytes(ctxs) // BLOWFISH_CTX_BYTES, _ptr(ctx_index), _ptr(words), _ptr(word_offsets),
              _ptr(block_counts), n, flags, h), fn.__name__)
    return words


def blowfish_encrypt_batch_keyed(ctxs, words, word_offsets, block_counts, ctx_index=None, stream=None, async_=False,
                                 all_devices=False):
    """BRB_Blowfish_EncryptBatchKeyed: record i = block_counts[i] (xl, xr) pairs at words[word_offsets[i]:],
    encrypted in place with ctxs[ctx_index[i]] (ctx_index None: ctxs[i]).  Returns words."""
    return _bf_keyed(lib().BRB_Blowfish_EncryptBatchKeyed, ctxs, words, word_offsets, block_counts, ctx_index, stream,
                     async_, all_devices)


def blowfish_decrypt_batch_keyed(ctxs, words, word_offsets, block_counts, ctx_index=None, stream=None, async_=False,
                                 all_devices=False):
    """BRB_Blowfish_DecryptBatchKeyed (see blowfish_encrypt_batch_keyed)."""
    return _bf_keyed(lib().BRB_Blowfish_DecryptBatchKeyed, ctxs, words, word_offsets, block_counts, ctx_index, stream,
                     async_, all_devices)


def device_count() -> int:
    """BRB_CryptoGPU_DeviceCount (0 without a usable device)."""
    return int(lib().BRB_CryptoGPU_DeviceCount())


# ---- RC4 and the RC4+MD5 frame ---------------------------------------------------
def rc4_init(key: bytes, keylen: int | None = None) -> BRB_RC4_State:
    """BRB_RC4_Init into a zeroed state."""
    st = BRB_RC4_State()
    kb = ctypes.create_string_buffer(bytes(key), max(len(key), 1))
    lib().BRB_RC4_Init(ctypes.byref(st), kb, len(key) if keylen is None else keylen)
    return st


def rc4_state_bytes(st: BRB_RC4_State) -> bytes:
    return ctypes.string_at(ctypes.addressof(st), RC4_STATE_BYTES)


def rc4_states(keys) -> np.ndarray:
    """(n, 264) uint8 array of BRB_RC4_Init states, one per key (the batch calls' `states`)."""
    out = np.empty((len(keys), RC4_STATE_BYTES), np.uint8)
    for i, k in enumerate(keys):
        out[i] = np.frombuffer(rc4_state_bytes(rc4_init(k)), np.uint8)
    return out


def _same_kind(ref, *xs):
    for x in xs:
        if x is not None and _is_torch(x) != _is_torch(ref):
            raise ValueError("all buffers of one batch call must be numpy (host) or all CUDA tensors (device)")


# ---- key setup as a batch (EvAIOReqTransform_CryptoEnable for many keys) ---------------------------
BLOWFISH_CTX_BYTES = 8336


def pack_keys(keys):
    """A list of `bytes` keys -> (blob uint8[sum], key_offsets uint64[n], key_lengths uint32[n]), the keys
    back to back in list order (so every offset residue mod 4 occurs with odd lengths)."""
    lens = np.array([len(k) for k in keys], np.uint32)
    offs = np.zeros(len(keys), np.uint64)
    if len(keys) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8).copy()
    return blob, offs, lens


def unpack_keys(blob, key_offsets, key_lengths):
    """The inverse of pack_keys for any layout (shared or overlapping keys included): a list of bytes."""
    raw = np.asarray(blob, np.uint8).tobytes()
    return [raw[int(o):int(o) + int(n)] for o, n in zip(key_offsets, key_lengths)]


def _init_batch(fn, width, keys, key_offsets, key_lengths, out, stream, async_, all_devices):
    _same_kind(keys, key_offsets, key_lengths, out)
    n = len(key_offsets)
    if len(key_lengths) != n:
        raise ValueError("key_offsets and key_lengths differ in length")
    if out is None:
        out = _out_like(keys, n, width)
    elif _nbytes(out) < n * width:
        raise ValueError(f"out holds {_nbytes(out)} bytes, {n} records need {n * width}")
    flags, h = _mode(keys, stream, async_, all_devices)
    _check(fn(_ptr(out), _ptr(keys), _ptr(key_offsets), _ptr(key_lengths), n, flags, h), fn.__name__)
    return out


def rc4_init_batch(keys, key_offsets, key_lengths, out=None, stream=None, async_=False, all_devices=False):
    """BRB_RC4_InitBatch: (n, 264) uint8 states, state i = zeroed + BRB_RC4_Init(keys[key_offsets[i]:
    +key_lengths[i]]).  keys uint8, key_offsets uint64[n], key_lengths uint32[n] (pack_keys): numpy for
    host mode, CUDA tensors for device mode (offsets int64, lengths int32)."""
    return _init_batch(lib().BRB_RC4_InitBatch, RC4_STATE_BYTES, keys, key_offsets, key_lengths, out, stream, async_,
                       all_devices)


def blowfish_init_batch(keys, key_offsets, key_lengths, out=None, stream=None, async_=False, all_devices=False):
    """BRB_Blowfish_InitBatch: (n, 8336) uint8 contexts, row i = BRB_Blowfish_Init of key i; a row of a
    device-mode result is the `ctx` of blowfish_encrypt_batch / blowfish_decrypt_batch as it stands."""
    return _init_batch(lib().BRB_Blowfish_InitBatch, BLOWFISH_CTX_BYTES, keys, key_offsets, key_lengths, out, stream,
                       async_, all_devices)


def rc4_crypt_batch(states, data, offsets, lengths, out=None, stream=None, async_=False, all_devices=False):
    """BRB_RC4_CryptBatch: stream i = data[offsets[i]:+lengths[i]] -> out (in place when out is None).
    states: (n, 264) uint8, updated in place."""
    out = data if out is None else out
    _same_kind(data, states, out, offsets, lengths)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_RC4_CryptBatch(_ptr(states), _ptr(data), _ptr(out), _ptr(offsets), _ptr(lengths), len(offsets),
                                    flags, h), "BRB_RC4_CryptBatch")
    return out


def rc4md5_frame_batch(states, payload, offsets, lengths, salts, frames, frame_offsets, stream=None, async_=False,
                       all_devices=False):
    """BRB_RC4MD5_FrameBatch: frames[frame_offsets[i]:+30+lengths[i]] = RC4(salt|"HASH:"|MD5|NUL|payload)."""
    _same_kind(payload, states, offsets, lengths, salts, frames, frame_offsets)
    flags, h = _mode(payload, stream, async_, all_devices)
    _check(lib().BRB_RC4MD5_FrameBatch(_ptr(states), _ptr(payload), _ptr(offsets), _ptr(lengths), _ptr(salts),
                                       _ptr(frames), _ptr(frame_offsets), len(offsets), flags, h),
           "BRB_RC4MD5_FrameBatch")
    return frames


def rc4md5_open_batch(states, frames, offsets, lengths, out=None, valid=None, stream=None, async_=False,
                      all_devices=False):
    """BRB_RC4MD5_OpenBatch: decrypt frames (in place when out is None); returns (out, valid uint8[n])."""
    out = frames if out is None else out
    n = len(offsets)
    if valid is None:
        valid = _out_like(frames, n, 1).reshape(n)
    _same_kind(frames, states, out, offsets, lengths, valid)
    flags, h = _mode(frames, stream, async_, all_devices)
    _check(lib().BRB_RC4MD5_OpenBatch(_ptr(states), _ptr(frames), _ptr(out), _ptr(offsets), _ptr(lengths), n,
                                      _ptr(valid), flags, h), "BRB_RC4MD5_OpenBatch")
    return out, valid


def rc4_crypt_list_batch(states, data, buf_offsets, buf_lengths, stream_first_buf, out=None, stream=None, async_=False,
                         all_devices=False):
    """BRB_RC4_CryptListBatch: stream i owns buffers stream_first_buf[i] .. stream_first_buf[i + 1] - 1
    (len(states) + 1 uint64 entries); buffer k = data[buf_offsets[k]:+buf_lengths[k]] -> out (in place when
    out is None).  states: (n, 264) uint8, each loaded and stored once."""
    out = data if out is None else out
    _same_kind(data, states, out, buf_offsets, buf_lengths, stream_first_buf)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_RC4_CryptListBatch(_ptr(states), _ptr(data), _ptr(out), _ptr(buf_offsets), _ptr(buf_lengths),
                                        _ptr(stream_first_buf), len(stream_first_buf) - 1, flags, h),
           "BRB_RC4_CryptListBatch")
    return out


def rc4md5_frame_list_batch(states, payload, buf_offsets, buf_lengths, salts, frames, frame_offsets, stream_first_buf,
                            stream=None, async_=False, all_devices=False):
    """BRB_RC4MD5_FrameListBatch: rc4md5_frame_batch with a buffer list per stream (salts and frame_offsets
    per buffer)."""
    _same_kind(payload, states, buf_offsets, buf_lengths, salts, frames, frame_offsets, stream_first_buf)
    flags, h = _mode(payload, stream, async_, all_devices)
    _check(lib().BRB_RC4MD5_FrameListBatch(_ptr(states), _ptr(payload), _ptr(buf_offsets), _ptr(buf_lengths),
                                           _ptr(salts), _ptr(frames), _ptr(frame_offsets), _ptr(stream_first_buf),
                                           len(stream_first_buf) - 1, flags, h), "BRB_RC4MD5_FrameListBatch")
    return frames


def rc4md5_open_list_batch(states, frames, buf_offsets, buf_lengths, stream_first_buf, out=None, valid=None, stream=None,
                           async_=False, all_devices=False):
    """BRB_RC4MD5_OpenListBatch: rc4md5_open_batch with a buffer list per stream; returns (out, valid uint8
    per buffer)."""
    out = frames if out is None else out
    nbuf = len(buf_offsets)
    if valid is None:
        valid = _out_like(frames, nbuf, 1).reshape(nbuf)
    _same_kind(frames, states, out, buf_offsets, buf_lengths, stream_first_buf, valid)
    flags, h = _mode(frames, stream, async_, all_devices)
    _check(lib().BRB_RC4MD5_OpenListBatch(_ptr(states), _ptr(frames), _ptr(out), _ptr(buf_offsets), _ptr(buf_lengths),
                                          _ptr(stream_first_buf), len(stream_first_buf) - 1, _ptr(valid), flags, h),
           "BRB_RC4MD5_OpenListBatch")
    return out, valid


RC4_KIND_CRYPT, RC4_KIND_FRAME, RC4_KIND_OPEN = 0, 1, 2   # BRB_RC4_KIND_*


def rc4_mixed_list_batch(states, stream_kind, data, buf_offsets, buf_lengths, out_offsets, stream_first_buf, out=None,
                         salts=None, valid=None, state_index=None, stream=None, async_=False):
    """BRB_RC4_MixedListBatch: stream i is of stream_kind[i] (RC4_KIND_*, uint8) and uses
    states[state_index[i]] (uint32; None: states[i]); buffer k = data[buf_offsets[k]:+buf_lengths[k]] ->
    out[out_offsets[k]:] (out None: data itself, for calls that work in place), 30 bytes longer for a FRAME
    stream.  salts (uint64 per buffer) is read for FRAME buffers, valid (uint8 per buffer) written for OPEN
    buffers; either may be None when no stream is of that kind.  Streams of one kind should be adjacent: a
    wave of 64 streams runs every kind it holds, one after another.  Returns (out, valid)."""
    out = data if out is None else out
    _same_kind(data, states, stream_kind, out, buf_offsets, buf_lengths, out_offsets, stream_first_buf, salts, valid,
               state_index)
    flags, h = _mode(data, stream, async_)
    _check(lib().BRB_RC4_MixedListBatch(_ptr(states), _nbytes(states) // RC4_STATE_BYTES, _ptr(state_index),
                                        _ptr(stream_kind), _ptr(data), _ptr(out), _ptr(buf_offsets), _ptr(buf_lengths),
                                        _ptr(out_offsets), _ptr(salts), _ptr(stream_first_buf),
                                        len(stream_first_buf) - 1, _ptr(valid), flags, h), "BRB_RC4_MixedListBatch")
    return out, valid


# ---- MemBuffer Blowfish ------------------------------------------------------------
def membuf_span(data_size: int) -> int:
    """BRB_MEMBUF_SPAN: bytes a call touches after buf + offset; data_size = size + offset to
    encrypt, size - offset to decrypt (mem_buf.c:1503, :1557)."""
    return ((data_size // 8 + 3) // 2) * 16


def membuf_key(seed: int) -> bytes:
    k = (ctypes.c_uint * 16)()
    lib().BRB_MemBufferKey(seed, k)
    return bytes(k)


def _membuf(fn, buf, size, seed, offset, stream, decrypt):
    need = offset + membuf_span(size - offset if decrypt else size + offset)
    if _nbytes(buf) < need:
        raise ValueError(f"buffer holds {_nbytes(buf)} bytes, the call needs {need}")
    flags, h = _mode(buf, stream, False)
    ns = ctypes.c_ulong(0)
    _check(fn(_ptr(buf), size, seed, offset, ctypes.byref(ns), flags, h), fn.__name__)
    return ns.value


def membuf_encrypt(buf, size, seed, offset=0, stream=None):
    """BRB_MemBufferEncrypt in place; returns the new MemBuffer size."""
    return _membuf(lib().BRB_MemBufferEncrypt, buf, size, seed, offset, stream, False)


def membuf_decrypt(buf, size, seed, offset=0, stream=None):
    """BRB_MemBufferDecrypt in place; returns the new MemBuffer size."""
    return _membuf(lib().BRB_MemBufferDecrypt, buf, size, seed, offset, stream, True)


def _membuf_batch(fn, data, buf_offsets, sizes, seeds, offsets, seed_index, new_sizes, stream, all_devices):
    seeds = np.ascontiguousarray(np.atleast_1d(seeds), np.uint32)      # always host memory: a parameter
    n = len(buf_offsets)
    if len(sizes) != n or (offsets is not None and len(offsets) != n) or (seed_index is not None and len(seed_index) != n):
        raise ValueError("buf_offsets, sizes, offsets and seed_index differ in length")
    if new_sizes is None:
        if _is_torch(data):
            import torch
            new_sizes = torch.zeros(n, dtype=torch.int64, device=data.device)
        else:
            new_sizes = np.zeros(n, np.uint64)
    _same_kind(data, buf_offsets, sizes, offsets, seed_index, new_sizes)
    flags, h = _mode(data, stream, False, all_devices)
    _check(fn(_ptr(data), _ptr(buf_offsets), _ptr(sizes), _ptr(offsets), _ptr(seeds), len(seeds), _ptr(seed_index), n,
              _ptr(new_sizes), flags, h), fn.__name__)
    return new_sizes


def membuf_encrypt_batch(data, buf_offsets, sizes, seeds, offsets=None, seed_index=None, new_sizes=None, stream=None,
                         all_devices=False):
    """BRB_MemBufferEncryptBatch in place: buffer i = data[buf_offsets[i]:] with MemBuffer size sizes[i], offset
    argument offsets[i] (None: 0) and seed seeds[seed_index[i]] (seed_index None: one seed for all, or one per
    buffer).  buf_offsets, sizes, offsets uint64[n], seed_index uint32[n]: numpy with numpy data, CUDA tensors
    (int64 / int32) with a CUDA tensor; seeds is a host sequence either way.  The caller has grown every buffer
    to membuf_span.  Returns new_sizes (uint64[n] numpy, or an int64 tensor)."""
    return _membuf_batch(lib().BRB_MemBufferEncryptBatch, data, buf_offsets, sizes, seeds, offsets, seed_index, new_sizes,
                         stream, all_devices)


def membuf_decrypt_batch(data, buf_offsets, sizes, seeds, offsets=None, seed_index=None, new_sizes=None, stream=None,
                         all_devices=False):
    """BRB_MemBufferDecryptBatch in place (see membuf_encrypt_batch); returns new_sizes."""
    return _membuf_batch(lib().BRB_MemBufferDecryptBatch, data, buf_offsets, sizes, seeds, offsets, seed_index, new_sizes,
                         stream, all_devices)


# ---- base64 -------------------------------------------------------------------------
def base64_encode_batch(data, offsets, lengths, out, out_offsets, stream=None, async_=False, all_devices=False):
    """BRB_Base64EncodeBatch: out[out_offsets[i]:+4*ceil(len/3)] = base64 of record i."""
    _same_kind(data, offsets, lengths, out, out_offsets)
    flags, h = _mode(data, stream, async_, all_devices)
    _check(lib().BRB_Base64EncodeBatch(_ptr(data), _ptr(offsets), _ptr(lengths), len(offsets), _ptr(out),
                                       _ptr(out_offsets), flags, h), "BRB_Base64EncodeBatch")
    return out


def base64_decode_batch(text, offsets, lengths, out, out_offsets, out_lengths=None, stream=None, async_=False,
                        all_devices=False):
    """BRB_Base64DecodeBatch: returns out_lengths (uint32[n])."""
    n = len(offsets)
    if out_lengths is None:
        if _is_torch(text):
            import torch
            out_lengths = torch.zeros(n, dtype=torch.int32, device=text.device)
        else:
            out_lengths = np.zeros(n, np.uint32)
    _same_kind(text, offsets, lengths, out, out_offsets, out_lengths)
    flags, h = _mode(text, stream, async_, all_devices)
    _check(lib().BRB_Base64DecodeBatch(_ptr(text), _ptr(offsets), _ptr(lengths), n, _ptr(out), _ptr(out_offsets),
                                       _ptr(out_lengths), flags, h), "BRB_Base64DecodeBatch")
    return out_lengths


# ---- receive-loop batching ---------------------------------------------------------
CRYPTO_FUNC_RC4, CRYPTO_FUNC_RC4_MD5 = 1, 2
BATCHER_ZERO_COPY = 0x100
BATCHER_PIPELINED = 0x200    # BRB_BATCHER_PIPELINED: two arenas, flush_async()
BATCHER_ALL_DEVICES = 0x400  # BRB_BATCHER_ALL_DEVICES: connections partitioned over the devices
BATCHER_CONN_LISTS = 0x800   # BRB_BATCHER_CONN_LISTS: one launch per direction, a buffer list per connection
BATCHER_MIXED = 0x1000       # BRB_BATCHER_MIXED: an algo per connection, one launch per round
OP_READ, OP_WRITE = 0, 1
TransformDone = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                                 ctypes.c_int)


class HostRegion:
    """Page-aligned host memory page-locked for the GPU (BRB_CryptoGPU_HostRegister)."""

    def __init__(self, size: int):
        import mmap
        self._L = lib()
        self.size = size
        self._mm = mmap.mmap(-1, size)
        self._view = (ctypes.c_char * size).from_buffer(self._mm)
        self.addr = ctypes.addressof(self._view)
        _check(self._L.BRB_CryptoGPU_HostRegister(self.addr, size), "BRB_CryptoGPU_HostRegister")

    def close(self):
        if self._mm is not None:
            self._L.BRB_CryptoGPU_HostUnregister(self.addr)
            del self._view
            self._mm.close()
            self._mm = None

    def __del__(self):
        self.close()


class TransformBatcher:
    """BRB_TransformBatcher*: one event-loop round of many connections per GPU call.

    zero_copy=True creates the batcher with BRB_BATCHER_ZERO_COPY: the kernels read each buffer in
    place from page-locked host memory.  This wrapper plays the part of a receive loop whose socket
    buffers are page-locked: it keeps one registered region and places each submitted buffer in it
    (the batcher itself copies nothing).

    pipelined=True creates it with BRB_BATCHER_PIPELINED: flush_async() starts the round and returns
    the previous round's results; flush() drains both.  In zero-copy mode the wrapper then keeps one
    region per arena, since a running round's buffers must stay unchanged until delivered.

    conn_lists=True creates it with BRB_BATCHER_CONN_LISTS: a round is one launch per direction, each
    connection's buffers a list walked between one load and one store of its state.

    mixed=True creates it with BRB_BATCHER_MIXED: `algo` is only the default, enable(conn, key, algo) gives
    a connection its own, and a round is one launch whatever the connections' algos."""

    def __init__(self, max_conns: int, max_round_bytes: int, algo: int = CRYPTO_FUNC_RC4_MD5, zero_copy: bool = False,
                 pipelined: bool = False, all_devices: bool = False, conn_lists: bool = False, mixed: bool = False):
        self._L = lib()
        n_reg = 2 if pipelined else 1
        self._regions = [HostRegion(max(max_round_bytes, 1)) for _ in range(n_reg)] if zero_copy else None
        self._cur = 0
        self._used = 0
        self.h = self._L.BRB_TransformBatcherCreate(max_conns, max_round_bytes,
                                                    algo | (BATCHER_ZERO_COPY if zero_copy else 0) |
                                                    (BATCHER_PIPELINED if pipelined else 0) |
                                                    (BATCHER_ALL_DEVICES if all_devices else 0) |
                                                    (BATCHER_CONN_LISTS if conn_lists else 0) |
                                                    (BATCHER_MIXED if mixed else 0))
        if not self.h:
            raise RuntimeError("BRB_TransformBatcherCreate: " + self._L.BRB_CryptoGPU_LastError().decode())

    def close(self):
        if self.h:
            self._L.BRB_TransformBatcherDestroy(self.h)
            self.h = None
        if self._regions is not None:
            for r in self._regions:
                r.close()
            self._regions = None

    def _place(self, data: bytes):
        """Zero-copy mode: the buffer's address inside the registered region (None when full)."""
        n = len(data)
        region = self._regions[self._cur]
        if self._used + n > region.size:
            return None
        a = region.addr + self._used
        ctypes.memmove(a, bytes(data), n)
        self._used += n
        return a

    def __del__(self):
        self.close()

    def enable(self, conn: int, key: bytes, algo: int | None = None):
        """BRB_TransformBatcherEnable; with algo, BRB_TransformBatcherEnableAlgo (the connection's own algo)."""
        if algo is not None:
            _check(self._L.BRB_TransformBatcherEnableAlgo(self.h, conn, algo, bytes(key), len(key)),
                   "BRB_TransformBatcherEnableAlgo")
            return
        _check(self._L.BRB_TransformBatcherEnable(self.h, conn, bytes(key), len(key)), "BRB_TransformBatcherEnable")

    def disable(self, conn: int):
        """BRB_TransformBatcherDisable: both states zeroed, read / write refuse the connection until enable."""
        _check(self._L.BRB_TransformBatcherDisable(self.h, conn), "BRB_TransformBatcherDisable")

    def enable_batch(self, conns, keys, algos=None):
        """BRB_TransformBatcherEnableBatch: connection conns[i] gets keys[i] (bytes), read and write
        state, in one GPU call.  With algos (one per connection), BRB_TransformBatcherEnableBatchAlgo."""
        if len(conns) != len(keys):
            raise ValueError("conns and keys differ in length")
        ids = np.ascontiguousarray(conns, np.uint32)
        blob, offs, lens = pack_keys(keys)
        if blob.size == 0:
            blob = np.zeros(1, np.uint8)
        if algos is not None:
            if len(algos) != len(conns):
                raise ValueError("conns and algos differ in length")
            al = np.ascontiguousarray(algos, np.uint8)
            _check(self._L.BRB_TransformBatcherEnableBatchAlgo(self.h, _ptr(ids), len(ids), _ptr(al), _ptr(blob), _ptr(offs),
                                                               _ptr(lens)), "BRB_TransformBatcherEnableBatchAlgo")
            return
        _check(self._L.BRB_TransformBatcherEnableBatch(self.h, _ptr(ids), len(ids), _ptr(blob), _ptr(offs), _ptr(lens)),
               "BRB_TransformBatcherEnableBatch")

    def read(self, conn: int, data: bytes) -> int:
        if self._regions is not None:
            a = self._place(data)
            return 0 if a is None else self._L.BRB_TransformBatcherRead(self.h, conn, a, len(data))
        return self._L.BRB_TransformBatcherRead(self.h, conn, bytes(data), len(data))

    def write(self, conn: int, data: bytes, salt: int) -> int:
        if self._regions is not None:
            a = self._place(data)
            return 0 if a is None else self._L.BRB_TransformBatcherWrite(self.h, conn, a, len(data), salt)
        return self._L.BRB_TransformBatcherWrite(self.h, conn, bytes(data), len(data), salt)

    def _run(self, fn_name):
        res = []

        def cb(_user, conn, op, out, n, valid):
            res.append((conn, op, ctypes.string_at(out, n) if n else b"", valid))

        fn = TransformDone(cb)
        launched = self._used > 0
        rc = getattr(self._L, fn_name)(self.h, fn, None)
        if rc in (BATCH_DROPPED, BATCH_PARTIAL):
            # DROPPED: every buffer came back through its callback, those of the dropped round with
            # valid == TRANSFORM_DROPPED and no output.  PARTIAL: the parts that delivered did; the
            # others' rounds stay pending for the next flush.  Either way the delivered results ride
            # on the exception.
            err = RuntimeError(fn_name + ": " + self._L.BRB_CryptoGPU_LastError().decode())
            err.results = res
            err.code = rc
            if rc == BATCH_DROPPED:
                if fn_name.endswith("Async") and launched and self._regions is not None and len(self._regions) == 2:
                    self._cur ^= 1
                self._used = 0
            raise err
        if rc < 0 or (rc == 0 and self._L.BRB_CryptoGPU_LastError()):
            err = RuntimeError(fn_name + ": " + self._L.BRB_CryptoGPU_LastError().decode())
            err.results = res    # whatever callbacks fired before the failure
            err.code = rc
            raise err
        if fn_name.endswith("Async") and launched and self._regions is not None and len(self._regions) == 2:
            self._cur ^= 1      # the running round keeps its region until delivered
        self._used = 0
        return res

    def flush(self):
        """Returns [(conn, op, out bytes, valid)] in submission order (every round still pending)."""
        return self._run("BRB_TransformBatcherFlush")

    def flush_async(self):
        """Pipelined: starts this round, returns the previous round's [(conn, op, out, valid)]."""
        return self._run("BRB_TransformBatcherFlushAsync")

    def inject_fault(self, launch: int) -> None:
        """Test support: the `launch`-th kernel launch of every round fails (-1: off)."""
        _check(self._L.BRB_TransformBatcherInjectFault(self.h, launch), "BRB_TransformBatcherInjectFault")

    def state(self, conn: int, op: int) -> bytes:
        st = BRB_RC4_State()
        _check(self._L.BRB_TransformBatcherGetState(self.h, conn, op, ctypes.byref(st)), "BRB_TransformBatcherGetState")
        return rc4_state_bytes(st)
