"""The core feature functions; `adx_core` is exported here as well as from `.trend`."""
from .trend import adx_core

__all__ = ["adx_core"]
