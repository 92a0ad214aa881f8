"""ld_tools_amd -- MI355X (gfx950) engine for the pairwise-LD hot path of PlatonB/ld-tools.

Scope: ``backend/calc_ld.py`` as driven by ``ld_triangle`` / ``ld_area``.

    from ld_tools_amd.backend.calc_ld import calc_ld          # drop-in, same signature / dict
    from ld_tools_amd import PackedPanel, ld_triangle, ld_area

All arithmetic runs in libldx.so (HIP, C ABI in include/ldx.h); importing the package without
that library fails -- there is no CPU fallback.
"""
from ._lib import LdxError, version  # noqa: F401  (loads libldx.so or raises)
from .ops import AreaHits, LDScores, TriangleResult, ld_area, ld_from_counts, ld_score, ld_triangle, pair_counts  # noqa: F401
from .ops import Clumps, LDNeighbors, Pruned, ld_clump, ld_neighbors, ld_prune  # noqa: F401
from .ops import LDProduct, RidgeResult, ld_matvec, ld_ridge, prod_terms  # noqa: F401
from .ops import LDDecay, ld_decay  # noqa: F401
from .ops import LDBlocks, blocks_host, ld_blocks  # noqa: F401
from .ops import LDCross, LDRegions, cross_host, ld_cross, ld_regions, region_positions, split_host  # noqa: F401
from .ops import dosage_host  # noqa: F401
from .ops import LDBand, band_layout_host, cross_terms, ld_band, ld_cross_score  # noqa: F401
from .ops import LDRectHits, ld_rect, ld_rect_hits, rect_hits_host  # noqa: F401
from .ops import ld_rect_counts, pairwise_cell_host, pairwise_counts_host, pw_snp_stats  # noqa: F401
from .ops import LDEm, em_host, ld_em, ld_em_counts, ld_em_from_counts, ld_em_hits  # noqa: F401
from .ops import LDEmBand, em_snp_stats, ld_em_band  # noqa: F401
from .ops import (GabrielBlocks, LDCiBand, dprime_ci_host, gabriel_candidates_host, gabriel_kept_host,  # noqa: F401
                  gabriel_pick_host, ld_ci_from_counts, ld_dprime_ci, ld_gabriel_blocks)
from .ops import (RelatedPairs, SampleCounts, ibs_cell_host, ibs_matrix, king_cell_host, king_cutoff,  # noqa: F401
                  king_from_counts, king_kinship, sample_counts, sample_counts_host)
from .ops import (GrmResult, grm_cell_host, grm_cutoff, grm_weights, ld_grm, ld_grm_from_sums, ld_grm_host,  # noqa: F401
                  sample_wprod, sample_wprod_host)
from .ops import (GenoOperator, GenoProduct, SamplePCA, Scores, geno_matmul, geno_matmul_host, geno_quantize,  # noqa: F401
                  geno_rmatmul, geno_rmatmul_host, polygenic_score, polygenic_score_host, sample_pca, sample_pca_host)
from .ops import (GLM_FLAGS, GlmDesign, GlmResult, geno_counts_host, geno_snp_counts, glm_design, glm_linear_host,  # noqa: F401
                  glm_tail_host, ld_glm, ld_glm_host)
from .ops import (FIRTH_MODES, FIRTH_STOP, LOGIT_FLAGS, LogitDesign, LogitResult, ld_glm_logistic,  # noqa: F401
                  ld_glm_logistic_host, logit_design, logit_tail_host)
from .ops import (MODEL_FLAGS, MODEL_TESTS, QC_FLAGS, HardyResult, MissingResult, ModelResult, SampleQC,  # noqa: F401
                  fisher_exact_host, geno_group_counts, geno_group_counts_host, hwe_exact_host, ld_fisher_from_counts, ld_hardy,
                  ld_hwe_from_counts, ld_model, ld_model_from_counts, ld_test_missing, model_tests_host, sample_qc,
                  sample_qc_host, sample_qc_mask, snp_qc_mask)
from .ops import (EPI_DF, EPI_FLAGS, EPI_TESTS, EpiCells, EpiHits, EpiResult, EpiSummary, epi_allelic_host,  # noqa: F401
                  epi_boost_host, epi_chisq_bound, epi_counts_host, epi_tail_host, ld_epistasis, ld_epistasis_counts,
                  ld_epistasis_from_counts, ld_epistasis_hits)
from .ops import (MPERM_FLAGS, MPERM_TESTS, MpermResult, PermLabels, ld_mperm, ld_mperm_counts, ld_mperm_from_counts,  # noqa: F401
                  ld_mperm_host, mperm_emp2, mperm_stat_host, perm_labels, perm_labels_host)
from .panel import PackedPanel, encode_codes, select_index  # noqa: F401
from . import plink  # noqa: F401
from .plink import BedFile, bed_codes_host, codes_bed_host, read_covar, read_pheno, write_bfile  # noqa: F401

__all__ = ["PackedPanel", "encode_codes", "select_index", "ld_triangle", "ld_area", "pair_counts", "ld_from_counts",
           "TriangleResult", "AreaHits", "ld_score", "LDScores", "ld_neighbors", "LDNeighbors", "ld_clump", "Clumps",
           "ld_prune", "Pruned", "ld_decay", "LDDecay", "ld_blocks", "LDBlocks", "blocks_host", "ld_cross", "LDCross", "ld_regions", "LDRegions", "cross_host", "split_host",
           "region_positions", "ld_matvec", "LDProduct", "ld_ridge", "RidgeResult", "prod_terms", "dosage_host", "ld_band", "LDBand",
           "ld_cross_score", "band_layout_host", "cross_terms", "ld_rect", "ld_rect_hits", "LDRectHits", "rect_hits_host", "ld_rect_counts", "pairwise_counts_host", "pairwise_cell_host", "pw_snp_stats", "ld_em", "LDEm",
           "ld_em_hits", "ld_em_counts", "ld_em_from_counts", "em_host", "ld_em_band", "LDEmBand", "em_snp_stats", "ld_dprime_ci",
           "LDCiBand", "ld_gabriel_blocks", "GabrielBlocks", "ld_ci_from_counts", "dprime_ci_host", "gabriel_candidates_host",
           "gabriel_pick_host", "gabriel_kept_host", "sample_counts", "SampleCounts", "RelatedPairs", "king_kinship", "ibs_matrix",
           "sample_counts_host", "king_cell_host", "ibs_cell_host", "king_from_counts", "king_cutoff", "GenoOperator", "GenoProduct",
           "sample_wprod", "sample_wprod_host", "grm_weights", "grm_cell_host", "ld_grm", "ld_grm_host", "ld_grm_from_sums",
           "grm_cutoff", "GrmResult",
           "geno_quantize", "geno_matmul", "geno_rmatmul", "geno_matmul_host", "geno_rmatmul_host", "polygenic_score",
           "polygenic_score_host", "Scores", "sample_pca", "sample_pca_host", "SamplePCA", "geno_snp_counts", "geno_counts_host",
           "glm_design", "GlmDesign", "ld_glm", "ld_glm_host", "glm_linear_host", "glm_tail_host", "GlmResult", "GLM_FLAGS", "LdxError",
           "logit_design", "LogitDesign", "ld_glm_logistic", "ld_glm_logistic_host", "logit_tail_host", "LogitResult", "LOGIT_FLAGS",
           "FIRTH_MODES", "FIRTH_STOP",
           "geno_group_counts", "geno_group_counts_host", "ld_hwe_from_counts", "ld_fisher_from_counts", "ld_model_from_counts",
           "hwe_exact_host", "fisher_exact_host", "model_tests_host", "ld_hardy", "HardyResult", "ld_model", "ModelResult",
           "ld_test_missing", "MissingResult", "sample_qc", "sample_qc_host", "SampleQC", "snp_qc_mask", "sample_qc_mask",
           "QC_FLAGS", "MODEL_TESTS", "MODEL_FLAGS",
           "ld_epistasis", "ld_epistasis_hits", "ld_epistasis_counts", "ld_epistasis_from_counts", "EpiResult", "EpiHits",
           "EpiSummary", "EpiCells", "epi_counts_host", "epi_allelic_host", "epi_boost_host", "epi_tail_host", "epi_chisq_bound",
           "EPI_TESTS", "EPI_DF", "EPI_FLAGS",
           "ld_mperm", "ld_mperm_counts", "ld_mperm_from_counts", "ld_mperm_host", "mperm_stat_host", "mperm_emp2", "perm_labels",
           "perm_labels_host", "PermLabels", "MpermResult", "MPERM_TESTS", "MPERM_FLAGS",
           "version", "plink", "BedFile", "bed_codes_host", "codes_bed_host", "write_bfile", "read_pheno", "read_covar"]
