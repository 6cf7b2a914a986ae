def __getattr__(name):
    # the renderer's public names, resolved on first use (importing the package stays free of torch)
    if name in ("ObjCoordRenderer", "Mesh"):
        from . import render
        return getattr(render, name)
    if name in ("KeyField", "TrainableKeyField", "DensityField", "RadianceField", "TrainableRadianceField", "FeatureField"):
        from . import fields
        return getattr(fields, name)
    if name in ("sample_farthest_points", "thin_keys", "estimate_pointcloud_normals", "estimate_pointcloud_local_coord_frames"):
        from . import sampling
        return getattr(sampling, name)
    if name in ("export_keys", "collect_candidates", "extract_mesh"):
        from . import key_export
        return getattr(key_export, name)
    if name in ("view_correspondences", "clean_mesh_vertices", "ViewCorrespondences", "subsampled_normals"):
        from . import correspondences
        return getattr(correspondences, name)
    if name in ("PerspectiveCameras", "RayBundle", "NDCMultinomialRaysampler", "MonteCarloRaysampler", "sample_images_at_mc_locs",
                "EmissionAbsorptionRaymarcherStratified", "ImplicitRendererStratified"):
        from . import rays
        return getattr(rays, name)
    if name in ("contrastive_loss", "huber", "returnCrossEntropy", "returnCrossEntropy2", "returnCrossEntropyWithNeg",
                "distortion_loss", "mip360loss", "render_loss"):
        from . import losses
        return getattr(losses, name)
    if name in ("pose_train_step", "nerf_train_step"):
        from . import training
        return getattr(training, name)
    if name in ("PoseBatches", "CorrespondenceBank", "AugmentParams", "draw_params", "rotation_matrix_2d", "ColorParams",
                "draw_color_params"):
        from . import augment
        return getattr(augment, name)
    if name in ("Adam", "pose_optimizer", "nerf_optimizer"):
        from . import optim
        return getattr(optim, name)
    if name in ("generate_bop_realsamples", "training_views", "TrainingViews", "read_bop_frames", "extract_rt"):
        from . import ingest
        return getattr(ingest, name)
    if name == "marching_cubes":
        from . import ops
        return ops.marching_cubes
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
