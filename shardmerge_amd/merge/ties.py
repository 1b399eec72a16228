"""TiesMerge: TIES-Merging (Yadav et al., 2023) - trim each finetune's delta to its largest entries, elect a sign
per parameter by the weighted sum, merge the agreeing entries, add the result onto output_base_model.  The reference
has no such operator; the function is defined in include/shardmerge_hip.h (``smhip_ties_merge``) and runs in three
HIP kernels (csrc/sm_ties.hpp) behind ``Engine.ties_merge``.

Tensor routing is FourierMerge's: embeddings / final norm / head pass through from the ``is_input`` / ``is_output``
finetune, every block tensor is merged over the finetunes whose layer window covers it, each against its own base.
Only the block-tensor merge (``merge_block``) differs, and there is no shape pre-flight: a streaming operator
takes every shape and rank."""
from __future__ import annotations

import logging

from ..config import TIES_OPTION_DEFAULTS
from .base import MergeTensorsBase
from .fast_fourier import FourierMerge

logger = logging.getLogger(__name__)


class TiesMerge(FourierMerge):
    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        self.density = TIES_OPTION_DEFAULTS["density"]
        self.ties_lambda = TIES_OPTION_DEFAULTS["ties_lambda"]
        self.ties_normalize = TIES_OPTION_DEFAULTS["ties_normalize"]
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)     # (sets the YAML overrides)

    async def initialize(self):
        await MergeTensorsBase.initialize(self)          # no transform lengths to check

    def get_readme(self) -> str:
        models = "\n".join(f"- {m.model} (vs {m.base}, weight {m.alpha})" for m in self.config.finetune_merge)
        return (f"# TIES Merged Model\nBase: {self.config.output_base_model}\n"
                f"Method: TIES (trim, elect sign, merge), density {self.density:g}, lambda {self.ties_lambda:g}, "
                f"{'normalized by the agreeing weights' if self.ties_normalize else 'plain sum'}\n"
                f"Models merged:\n{models}\n")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.ties_merge(fts, bases, alphas, base_out, density=self.density, lam=self.ties_lambda,
                              normalize=bool(self.ties_normalize), layer_name=name)

    def block_cost_ms(self, shape, k: int) -> float:
        """the partitioned path's cost model: (2k + 3) streaming passes over the tensor"""
        numel = 1
        for d in shape:
            numel *= int(d)
        return 0.02 + 2.0 * numel * (2 * k + 3) / 4.0e9

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), TIES kept {report.kept} of {report.k_keep} asked, thresholds "
                    f"{[float(f'{t:.4g}') for t in report.thresholds]}")
