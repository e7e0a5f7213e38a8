"""waveformer_amd -- MI355X (gfx950) implementation of the WaveFormer encoder/decoder hot path.

`waveformer_amd.network_models` mirrors the reference `network_models` package (same class
names, constructor arguments and state_dict keys); its hot-path ops run on the HIP kernels of
`libwaveformer_hip.so` through the C-ABI in include/waveformer_hip.h.
"""
__version__ = "0.1.0"

__all__ = ["metrics", "region_metrics"]


def __getattr__(name):
    # evaluation (waveformer_amd.metrics) on first use: importing the package stays as light
    # as it was
    if name == "metrics":
        import importlib
        return importlib.import_module(".metrics", __name__)
    if name == "region_metrics":
        from .metrics import region_metrics
        return region_metrics
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
