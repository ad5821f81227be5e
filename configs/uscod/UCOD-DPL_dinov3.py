# UCOD-DPL first stage on DINOv3 ViT-B/16 features (HF DINOv3ViTModel: 4 register tokens, rotary position embedding): configs/uscod/UCOD-DPL_dinov2.py with
# another backbone and an image size that patch 16 divides.  The reference ships no such file; every other key and value is the DINOv2 file's.
_BACKBONE = {
    "type": "dinov3",
    "backbone": "facebook/dinov3-vitb16-pretrain-lvd1689m",
    "backbone_type": "huggingface",
    "backbone_weights": "./weights",
    "backbone_weight_base": "~/workspace/weights/huggingface",
    "backbone_feat_dim": [768],
}
_IMAGE = (512, 512)          # 512 / 16 = 32 x 32 patch grid

cfg = {
    "_BASE_": ["../__base__/accelerate.py", "../__base__/newbase.py", "../dataset/cod4040.py"],
    "exp_name": "UCOD-DPL_dinov3",
    "model_cfg": {"dim": 768, "feature_size": 68, "ema_weight": 0.99, "dis_use_features": False},
    "train_cfg": {
        "start_epoch": 0,
        "max_epoch": 25,
        "lr0": 2e-4,
        "step_lr_size": 25,
        "step_lr_gamma": 0.95,
        # discriminator phase: one epoch every second epoch
        "dis_epoch": 1,
        "dis_intertrain": 2,
        "dis_lr0": 1e-3,
        "dis_step_lr_size": 25,
        "dis_step_lr_gamma": 0.95,
    },
    "val_cfg": {"look_twice": True, "look_twice_th": 0.15, "expand_type": "dynamic", "val_interval": 5, "val_start": 5},
    "log_cfg": {"log_interval": 50},
    "dataset_cfg": {
        "cache_dir": "./datasets/cache",
        "trainset_cfg": {"DATASET": "TR-CAMO+TR-COD10K", "image_size": _IMAGE, "require_label": False, "bkg_th": 0.6},
        "valset_cfg": {"DATASET": "TE-CAMO", "image_size": _IMAGE, "require_label": True},
        "trainloader_cfg": {"batch_size": 16, "num_workers": 0, "shuffle": True},
        "val_loader_cfg": {"batch_size": 1, "num_workers": 0, "shuffle": False},
        "feature_extractor_cfg": _BACKBONE,
    },
}
