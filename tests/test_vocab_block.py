"""bofi_vocab_block and BOFI_FLAG_IDS_ONLY at the ABI level: declared, bound, exported, and bad arguments refused before anything touches a device."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_vocab_block_is_declared_bound_and_exported():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    assert "int bofi_vocab_block(" in header and "#define BOFI_FLAG_IDS_ONLY 8192" in header and "int bofi_engine_fork_ex(" in header
    assert "bofi_vocab_block" in hip.SIGNATURES and len(hip.SIGNATURES["bofi_vocab_block"][1]) == 18
    assert hip.FLAG_IDS_ONLY == 8192 and hip.FORK_IDS_ONLY == 1
    for name in ("bofi_vocab_block", "bofi_engine_fork_ex", "bofi_engine_ids_only_fused"):
        assert hasattr(lib, name), name
    assert callable(hip.vocab_block)


def test_vocab_block_refuses_bad_arguments_without_a_device():
    """Every one of these returns BOFI_ERR_ARG (1) from the argument check: the pointers are never read, no launch, no allocation."""
    _, lib = _lib()
    p = C.c_void_p(0x1000)              # (any non-null value: validation comes first)
    good = dict(x=p, ldx=512, wp=p, c=p, cs=p, M=4, Npad=128, V=100, S=2, ntok=None, ntok_bias=0, pad_idx=0, seq=p, plogp=p, chosen=p, nan=None, alone=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.bofi_vocab_block(a["x"], a["ldx"], a["wp"], a["c"], a["cs"], a["M"], a["Npad"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad_idx"], a["seq"],
                                    a["plogp"], a["chosen"], a["nan"], a["alone"], a["stream"])

    assert call(seq=None) == 1
    assert call(plogp=None) == 1 and call(chosen=None) == 1            # the two statistics: both or neither
    assert call(V=129) == 1                                            # V > Npad
    assert call(Npad=100) == 1 and call(Npad=32, V=20) == 1            # Npad % 64 != 0
    assert call(pad_idx=100) == 1 and call(pad_idx=-1) == 1            # pad_idx outside [0, V)
    assert call(x=None) == 1 and call(wp=None) == 1 and call(c=None) == 1 and call(cs=None) == 1
    assert call(M=0) == 1 and call(S=0) == 1 and call(V=0) == 1 and call(ldx=510) == 1
