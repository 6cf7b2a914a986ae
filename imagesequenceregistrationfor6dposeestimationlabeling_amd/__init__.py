def __getattr__(name):
    # the renderer's public names, resolved on first use (importing the package stays free of torch)
    if name in ("ObjCoordRenderer", "Mesh"):
        from . import render
        return getattr(render, name)
    if name == "KeyField":
        from . import fields
        return fields.KeyField
    if name in ("sample_farthest_points", "thin_keys"):
        from . import sampling
        return getattr(sampling, name)
    if name == "export_keys":
        from . import key_export
        return key_export.export_keys
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
