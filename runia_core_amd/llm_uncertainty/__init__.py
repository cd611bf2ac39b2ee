from .conformal import TokenConformal, TokenSets  # noqa: F401
from .consistency import (ConsistencyScores, PairCounts, consistency_scores, graph_scores, pairwise_counts,  # noqa: F401
                          pairwise_similarity, word_ids)
from .embedding_consistency import (EmbeddingSimilarity, embedding_consistency_scores,  # noqa: F401
                                    embedding_similarity)
from .llm_check import LLMCheckScores, attention_score, hidden_score, llm_check_scores  # noqa: F401
from .logit_lens import LogitLensScores, logit_lens  # noqa: F401
from .logits import GenerationScores, generation_scores, token_entropies, transition_scores  # noqa: F401
from .pipeline import compute_uncertainties, compute_uncertainties_batch, eigen_scores  # noqa: F401
from .rauq import (RAUQ, generated_lengths, rauq_batch, rauq_uncertainty, rauq_uncertainty_mean_heads,  # noqa: F401
                   rauq_uncertainty_rollout)
from .scores import eigen_score, semantic_entropy  # noqa: F401

__all__ = ["eigen_score", "semantic_entropy", "rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout",
           "RAUQ", "rauq_batch", "generated_lengths", "GenerationScores", "generation_scores", "token_entropies",
           "transition_scores", "compute_uncertainties", "compute_uncertainties_batch", "eigen_scores", "TokenConformal",
           "TokenSets", "PairCounts", "ConsistencyScores", "pairwise_counts", "pairwise_similarity", "graph_scores",
           "consistency_scores", "word_ids", "LLMCheckScores", "hidden_score", "attention_score", "llm_check_scores",
           "LogitLensScores", "logit_lens", "EmbeddingSimilarity", "embedding_similarity", "embedding_consistency_scores"]
