"""deseq2_amd -- MI355X-native per-gene NB-GLM engine behind DESeq2's fitBeta / fitDisp /
fitDispGrid boundary.  The compute lives in libdeseq2_mi355x.so
(hand-written HIP for gfx950); this package is the host-side mirror of the reference's R
callers of that boundary."""
from . import _lib  # noqa: F401
from .native import fitBeta, fitDisp, fitDispGrid  # noqa: F401
from .core import estimateSizeFactors, estimateSizeFactorsForMatrix  # noqa: F401
from .core import (vst, varianceStabilizingTransformation, getVarianceStabilizedData, normTransform,  # noqa: F401
                   normalized_counts, DESeqTransform)
from .core import results, resultsContrasts, resultsNames, DESeqResults, p_adjust, pvalueAdjustment, lowess  # noqa: F401
from .core import pt  # noqa: F401
from .core import unmix  # noqa: F401
from .core import apeglm, lfcShrinkApeglm, svalue, apeglm_prior_scale  # noqa: F401
from .core import ash, lfcShrinkAshr  # noqa: F401
from .core import rowVars, sampleDists, pca, plotPCA, PCAData  # noqa: F401
from .core import collapseReplicates, fpm, fpkm, counts, plotCounts  # noqa: F401
from .core import localDispersionFit  # noqa: F401

__all__ = ["fitBeta", "fitDisp", "fitDispGrid", "estimateSizeFactors", "estimateSizeFactorsForMatrix", "vst",
           "varianceStabilizingTransformation", "getVarianceStabilizedData", "normTransform", "normalized_counts",
           "DESeqTransform", "results", "resultsContrasts", "resultsNames", "DESeqResults", "p_adjust", "pvalueAdjustment", "lowess",
           "pt", "unmix", "rowVars", "sampleDists", "pca", "plotPCA", "PCAData", "collapseReplicates", "fpm", "fpkm", "counts",
           "plotCounts", "localDispersionFit"]
