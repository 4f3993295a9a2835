"""Importing this package registers `HAT`, `HATX`, `HybridHATNAF`, `ESC`, `ESCReal`, `ESCRealM`, `ESCFP`, `ESCLTE` (the arbitrary-scale model), `SRVGGNetCompact` and `RRDBNet` under their names (hat/archs/__init__.py:8-11
does the same by scanning `*_arch.py`)."""
from .hat_arch import HAT  # noqa: F401
from .hybrid_hat_naf_arch import HybridHATNAF  # noqa: F401
from .esc_arch import ESC  # noqa: F401
from .esc_real_arch import ESCReal  # noqa: F401
from .esc_real_m_arch import ESCRealM  # noqa: F401
from .esc_fp_arch import ESCFP  # noqa: F401
from .esc_lte_arch import ESCLTE  # noqa: F401
from .srvgg_arch import SRVGGNetCompact  # noqa: F401
from .rrdbnet_arch import RRDBNet  # noqa: F401
