"""Merge operators behind the reference's MergeTensorsBase interface."""
from importlib import import_module

# merge_options.operator -> (module, class); the module is imported when the operator is asked for
_OPERATOR_CLASSES = {
    "fourier": ("fast_fourier", "FourierMerge"),
    "addition": ("addition", "AdditionMerge"),
    "task_addition": ("taskaddition", "TaskAdditionMerge"),
    "fourier_legacy": ("fourier_legacy", "LegacyFourierMerge"),
    "ties": ("ties", "TiesMerge"),
    "dare_ties": ("dare", "DareTiesMerge"),
    "dare_linear": ("dare", "DareLinearMerge"),
    "breadcrumbs": ("breadcrumbs", "BreadcrumbsMerge"),
    "breadcrumbs_ties": ("breadcrumbs", "BreadcrumbsTiesMerge"),
    "model_stock": ("geometric", "ModelStockMerge"),
    "nuslerp": ("geometric", "NuSlerpMerge"),
    "slerp": ("geometric", "SlerpMerge"),
    "sce": ("sce", "SceMerge"),
    "della": ("della", "DellaMerge"),
    "della_linear": ("della", "DellaLinearMerge"),
    "consensus_ta": ("consensus", "ConsensusTaMerge"),
    "consensus_ties": ("consensus", "ConsensusTiesMerge"),
    "karcher": ("spherical", "KarcherMerge"),
    "multislerp": ("spherical", "MultiSlerpMerge"),
    "arcee_fusion": ("fusion", "ArceeFusionMerge"),
    "nearswap": ("fusion", "NearSwapMerge"),
    "pcb": ("pcb", "PcbMerge"),
    "tsv": ("tsv", "TsvMerge"),
    "widen": ("widen", "WidenMerge"),
    "cabs": ("cabs", "CabsMerge"),
    "iso_c": ("iso", "IsoMerge"),
    "emr": ("emr", "EmrMerge"),
}


def operator_class(name: str = "fourier"):
    """merge_options.operator -> class (the reference CLI hard-wires FourierMerge, __main__.py:22,67)."""
    if name not in _OPERATOR_CLASSES:
        raise ValueError(f"unknown merge operator {name!r}")
    module, cls = _OPERATOR_CLASSES[name]
    return getattr(import_module(f".{module}", __name__), cls)
