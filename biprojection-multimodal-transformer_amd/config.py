"""Process-wide defaults of the MI355X build (not reference flags)."""
import os

from ._lib import BPM_BF16, BPM_F32

PRECISIONS = ("bf16", "f32", "bf16x3")
_PRECISION = os.environ.get("BPMULT_PRECISION", "bf16")


def set_precision(name: str) -> None:
    """'bf16' (throughput: bf16 MFMA operands, f32 accumulate / residual stream), 'f32' (parity: exact f32 MFMA end to
    end) or 'bf16x3' (parity-grade and faster than f32: everything as in f32 mode except the large linear-layer products,
    which run as three bf16 MFMA products of split operands -- ~2^-16 relative per product).  Read when a model first runs."""
    global _PRECISION
    if name not in PRECISIONS:
        raise ValueError("precision must be 'bf16', 'f32' or 'bf16x3'")
    _PRECISION = name


def precision() -> str:
    return _PRECISION


_DETERMINISTIC = os.environ.get("BPMULT_DETERMINISTIC", "0") not in ("", "0")


def set_deterministic(flag: bool) -> None:
    """Deterministic mode ("Deterministic mode"): every launch of forward, backward and FusedAdam.step leaves
    the same bits on every run -- no float atomics: the linear layers' bias gradients ride on their weight-gradient
    products (colsum_a), the row kernels' column sums go through partial-row workspaces.  Off by default; the default
    path is unchanged by it.  Read where launch tables and plans are BUILT (a model's first forward at a batch size, a
    captured graph), never per launch: switch it before, or call model.set_deterministic()."""
    global _DETERMINISTIC
    _DETERMINISTIC = bool(flag)


def deterministic() -> bool:
    return _DETERMINISTIC


def resolve_deterministic(flag) -> bool:
    """A module's or argument's `deterministic` value: None means the process default."""
    return _DETERMINISTIC if flag is None else bool(flag)


def dtype_code(name: str) -> int:
    """Storage / compute type of the activations and weight shadows (bf16x3 keeps fp32 storage)."""
    if name not in PRECISIONS:
        raise ValueError(f"unknown precision {name!r}")
    return BPM_BF16 if name == "bf16" else BPM_F32


def is_x3(name: str) -> bool:
    return name == "bf16x3"
