_EXPORTS = {"read_depth_gt": "groundtruth", "read_pfm": "groundtruth", "read_npy": "groundtruth", "GtError": "groundtruth",
            "ImageDataset": "datasets", "UnrealStereo4kDataset": "datasets", "collate_train": "datasets"}


def __getattr__(name):          # resolved on first use: importing the package stays free of torch and of the HIP library
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module(f".{_EXPORTS[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
