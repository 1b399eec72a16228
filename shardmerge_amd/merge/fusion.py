"""ArceeFusionMerge / NearSwapMerge: the pairwise operators, after mergekit's ``arcee_fusion`` and ``nearswap`` (as recalled;
PAPERS.md) - ONE model is grafted onto its base, element by element.  ``arcee_fusion`` scores every row of a tensor by
the KL divergence of its softmax in the model from its softmax in the base, every element by ``|delta|`` times its row's
score, and takes the delta only where that exceeds ``median + fusion_iqr * (Q3 - Q1)`` of the tensor's scores;
``nearswap`` clamps the delta to ``[-nearswap_t, nearswap_t]``.  The reference has no such operator; the function is
defined in include/shardmerge_hip.h (``smhip_fusion_merge``) and runs in the HIP kernels of csrc/sm_fusion.hpp behind
``Engine.fusion_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs - and the
coverage rule: a pairwise operator fuses ONE model into a tensor, so every block tensor must be covered by exactly one
finetune_merge entry.  ``initialize`` checks it for every layer before anything is written."""
from __future__ import annotations

import logging

from ..config import FUSION_OPTION_DEFAULTS
from ..writer import ShardLayer
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class ArceeFusionMerge(TiesMerge):
    mode = "arcee"
    operator = "arcee_fusion"

    option_defaults = FUSION_OPTION_DEFAULTS

    async def initialize(self):
        await super().initialize()
        self.check_coverage()

    def check_coverage(self):
        """every block tensor under exactly one entry's layer window, else ValueError naming the layer and the entries"""
        layers = set()
        for name in self.index_manager.get_layer_order(self.config.output_base_model):
            try:
                number = ShardLayer(0, "", name, False).layer_number
            except ValueError:
                continue                      # (the merge itself reports unknown names, as the reference does)
            if number >= 0:
                layers.add(number)
        for number in sorted(layers):
            over = [m.model for m in self.config.finetune_merge if m.use_layer_index(number)]
            if len(over) != 1:
                raise ValueError(f"operator {self.operator} fuses ONE model into a tensor: layer {number} is covered by "
                                 f"{len(over)} finetune_merge entries ({', '.join(over) or 'none'}); give the entries disjoint "
                                 f"start_layer / end_layer windows that cover every layer once.  Nothing was written")

    def _method(self) -> str:
        return (f"Arcee Fusion (arcee_fusion: the delta where |delta| * KL(softmax(row) || softmax(base row)) exceeds "
                f"median + fusion_iqr * IQR of the tensor's scores), fusion_iqr {self.fusion_iqr:g}")

    def get_readme(self) -> str:
        models = "\n".join(f"- {m.model} (vs {m.base}" + (f", layers {m.start_layer}..{m.end_layer if m.end_layer != -1 else 'end'})"
                                                          if (m.start_layer, m.end_layer) != (0, -1) else ")")
                           for m in self.config.finetune_merge)
        return (f"# {'Arcee Fusion' if self.mode == 'arcee' else 'NearSwap'} Merged Model\nBase: {self.config.output_base_model}\n"
                f"Method: {self._method()}\nModel fused:\n{models}\n")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        if len(fts) != 1:
            raise ValueError(f"operator {self.operator} fuses ONE model into a tensor: {name} is covered by {len(fts)} entries")
        return eng.fusion_merge(fts[0], bases[0], base_out, mode=self.mode, iqr_mult=self.fusion_iqr, t=self.nearswap_t,
                                layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # the row KL 2, three selection levels of 2, the gate pass 4; nearswap: its one pass
        return 12 if self.mode == "arcee" else 4

    def _log_block(self, name: str, k: int, report):
        if self.mode == "arcee":
            logger.info(f"Merged {name}: Arcee Fusion selected {report.selected} of {report.n}, threshold {report.threshold:.4g} "
                        f"(quartiles {report.q1:.4g} / {report.q2:.4g} / {report.q3:.4g}), row KL {report.kl_min:.4g} .. {report.kl_max:.4g}")
        else:
            logger.info(f"Merged {name}: NearSwap clipped {report.clipped} of {report.n} at t {self.nearswap_t:g}")


class NearSwapMerge(ArceeFusionMerge):
    mode = "nearswap"
    operator = "nearswap"

    def _method(self) -> str:
        return f"NearSwap (nearswap: the delta clamped to [-t, t]), nearswap_t {self.nearswap_t:g}"
