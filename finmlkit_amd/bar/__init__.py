"""Bars from ticks.  The kits the reference does not have are exported here; they load with the first use, like every other module
of the package that is imported by its own path."""
__all__ = ["ImbalanceBarKit", "RunBarKit"]


def __getattr__(name):
    if name in __all__:
        from . import kit
        return getattr(kit, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
