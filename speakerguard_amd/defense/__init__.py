"""Defenses on the native engine, under the names the reference's defense/defense.py resolves (``Input_Transformation``)."""
from .feature_level import FEATURE_COMPRESSION, FeCo  # noqa: F401
from .time_domain import AS, AT, BDR, MS, QT  # noqa: F401
from .frequency_domain import BPF, DS, LPF  # noqa: F401
