"""The reference's ``--model`` factory for the accelerated models (src/definer.py:37-174):
``get_model(args) -> torch.nn.Module`` with the same Namespace fields (model, width, norm, act,
num_classes, dropout) and the same error behaviour (NameError for an unknown model), and its ``--criterion`` factory
(src/definer.py:177-288): ``make_criterion(args)`` with the Namespace fields criterion and num_classes, and its ``--optimizer``
factory (src/definer.py:291-380): ``make_optimizer(args, model)``."""
import argparse

import torch


def get_model(args: argparse.Namespace) -> torch.nn.Module:
    from .networks import EquiUnet

    kwargs = {
        "inplanes": 4,
        "num_classes": args.num_classes,
        "features": [args.width * 2 ** i for i in range(4)],
        "norm_layer": args.norm,
        "act": args.act,
        "deep_supervision": True,  # hard-wired in the reference factory, src/definer.py:140
        "dropout": args.dropout,
    }
    if args.model == "equiunet":
        return EquiUnet(**kwargs)
    if args.model == "equiunet_ref":  # src/definer.py:145-147
        return EquiUnet(**kwargs, refinement=True)
    if args.model in ("equiunet_assp_evo", "equiunet_assp_evocor"):
        from .networks.equiunet_assp import EquiUnetASSPEvo

        return EquiUnetASSPEvo(**kwargs)
    if args.model == "modified_unet":  # src/definer.py:155-170 (no dropout argument there)
        from .networks import Unet

        return Unet(img_ch=4, output_ch=args.num_classes, features=kwargs["features"], norm_layer=args.norm, act=args.act,
                    deep_supervision=True)
    raise NameError("Not Supported Model")  # (r2unet, r2attunet, att_unet of the same family included)


_MONAI_ONLY_CRITERIA = ("generalized_dice", "focal", "tversky", "dice_ce", "dice_focal")


def make_criterion(args: argparse.Namespace) -> torch.nn.Module:
    """src/definer.py:177-288 for the criteria built here, with the reference's own keyword sets: dice / jaccard (monai
    DiceLoss(sigmoid, squared_pred, batch=True) = losses.DiceLoss) and hd / dice_hd / boundary / dice_boundary
    (learning/losses.py).  The boundary criteria take the pair [target, distance_map] as their target."""
    from . import losses

    if args.criterion in ("dice", "jaccard"):
        return losses.DiceLoss(jaccard=args.criterion == "jaccard")
    if args.criterion == "hd":
        criterion_function = losses.HausdorffLoss
        kwargs = {
            "idc": list(range(args.num_classes)),
            "sigmoid": True,
            "softmax": False,
            "alpha": 2,
        }
    elif args.criterion == "dice_hd":
        criterion_function = losses.DiceHDLoss
        kwargs = {
            "idc_hd": list(range(args.num_classes)),
            "alpha_hd": 2,
            "hybrid": False,
            "include_background": True,
            "sigmoid": True,
            "softmax": False,
            "squared_pred": True,
            "weight_hd": 0.5,
            "weight_dice": 0.5,
        }
    elif args.criterion == "boundary":
        criterion_function = losses.BoundaryLoss
        kwargs = {
            "idc": list(range(args.num_classes)),
            "sigmoid": True,
            "softmax": False,
        }
    elif args.criterion == "dice_boundary":
        criterion_function = losses.DiceBoundaryLoss
        kwargs = {
            "idc_boundary": list(range(args.num_classes)),
            "include_background": True,
            "sigmoid": True,
            "softmax": False,
            "squared_pred": True,
        }
    elif args.criterion in _MONAI_ONLY_CRITERIA:
        raise NotImplementedError(f"--criterion {args.criterion} is MONAI's own loss and is not built here")
    else:
        raise NameError("Not Supported Criterion")
    kwargs["reduction"] = "mean"
    return criterion_function(**kwargs)


def make_optimizer(args: argparse.Namespace, model: torch.nn.Module) -> torch.optim.Optimizer:
    """src/definer.py:291-380 with the reference's own keyword sets: ranger -> optim.Ranger2020 (two launches per step), sgd /
    adam / adamw -> torch's.  The reference wraps the result for --adaptive_gradient_clipping itself (src/main_train.py:89-90):
    ``optim.AGC(model.parameters(), optimizer)``."""
    trainable = filter(lambda x: x.requires_grad, model.parameters())
    if args.optimizer == "sgd":
        optimizer_function = torch.optim.SGD
        kwargs = {"momentum": 0.9}
    elif args.optimizer in ("adam", "adamw"):
        optimizer_function = torch.optim.Adam if args.optimizer == "adam" else torch.optim.AdamW
        kwargs = {
            "betas": (0.9, 0.999),
            "eps": 1e-08,
        }
    elif args.optimizer == "ranger":
        from .optim import Ranger2020

        optimizer_function = Ranger2020
        kwargs = {
            "alpha": 0.5,
            "k": 6,
            "N_sma_threshhold": 5,
            "betas": (.95, 0.999),
            "eps": 1e-5,
            "weight_decay": 0,
            "use_gc": args.use_gc,
            "use_gcnorm": args.use_gcnorm,
            "normloss": args.normloss,
            "normloss_factor": args.normloss_factor,
            "gc_conv_only": args.gc_conv_only,
            "gc_loc": True,
        }
    elif args.optimizer in ("ranger21", "novograd"):
        raise NotImplementedError(f"--optimizer {args.optimizer} is a third-party package's optimizer and is not built here")
    else:
        raise NameError("Not Supported Optimizer")
    kwargs["lr"] = args.learning_rate
    kwargs["weight_decay"] = args.weight_decay
    return optimizer_function(trainable, **kwargs)
