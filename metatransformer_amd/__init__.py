"""metatransformer_amd -- MI355X-native Meta-Transformer encoder hot path.

Drop-in for the reference's `timm.models.vision_transformer.Block` stack and the Data2Seq tokenizers that
feed it (see encoder.py / data2seq.py); all compute runs in libmetaenc.so (hand-written HIP for gfx950)
behind the C ABI of include/metaenc.h.
"""
from ._capi import MetaEncError, load as load_library  # noqa: F401
from .encoder import (Attention, Block, Mlp, build_encoder, set_fp32_mode, convert_video_state_dict, encoder_flops_per_sample,  # noqa: F401
                      encoder_forward_inference, resize_pos_embed, to_video_state_dict)
from .heads import (ClassifierHead, ClsHead, FeaturePropogation, P3Embed, PointPatchEmbed, PointViTDecoder, PointViTPartDecoder,  # noqa: F401
                    SegHead, furthest_point_sample, group_features, knn_indices, load_encoder_checkpoint, pack_encoder, pool_tokens,
                    save_encoder_checkpoint, three_interpolation, three_nn)
from .adapter import (ConvFFN, DWConv, Extractor, Injector, InteractionBlock, MSDeformAttn, SpatialPriorModule, ViTAdapter,  # noqa: F401
                      conv3x3_rows, conv_transpose2x2_rows, deform_inputs, get_reference_points, max_pool3x3s2_rows, ms_deform_attn,
                      resize_rows_batched)
from .data2seq import (AcousticPatchEmbed, Data2Seq, DataEmbedding, GraphFeatureTokenizer, PatchEmbed, VideoPatchEmbed,  # noqa: F401
                       sinusoid_table, video_sinusoid_table)
from .timeseries import AttentionLayer, Decoder, DecoderLayer, Forecaster, FullAttention  # noqa: F401
from .hyperspectral import HyperSpectralClassifier, HyperSpectralEmbed, neighborhood_tokens  # noqa: F401
from .video_mae import (PretrainVisionTransformer, PretrainVisionTransformerDecoder, PretrainVisionTransformerEncoder,  # noqa: F401
                        mae_reconstruction_loss)
from .audio import ASTModel, KaldiFbank, fbank_tables, mel_filterbank, specaug_bands  # noqa: F401

__all__ = ["Block", "Attention", "Mlp", "build_encoder", "set_fp32_mode", "encoder_flops_per_sample", "encoder_forward_inference", "Data2Seq", "PatchEmbed",
           "AcousticPatchEmbed", "VideoPatchEmbed", "DataEmbedding", "MetaEncError", "load_library",
           "convert_video_state_dict", "to_video_state_dict", "resize_pos_embed", "ClassifierHead", "ClsHead", "PointPatchEmbed", "P3Embed",
           "furthest_point_sample", "knn_indices", "group_features", "pool_tokens",
           "FeaturePropogation", "PointViTDecoder", "PointViTPartDecoder", "SegHead", "three_nn", "three_interpolation", "load_encoder_checkpoint", "save_encoder_checkpoint", "pack_encoder",
           "ms_deform_attn", "MSDeformAttn", "Injector", "Extractor", "ConvFFN", "DWConv", "InteractionBlock", "deform_inputs", "get_reference_points",
           "conv3x3_rows", "max_pool3x3s2_rows", "resize_rows_batched", "conv_transpose2x2_rows", "SpatialPriorModule", "ViTAdapter",
           "GraphFeatureTokenizer", "FullAttention", "AttentionLayer", "DecoderLayer", "Decoder", "Forecaster",
           "HyperSpectralEmbed", "HyperSpectralClassifier", "neighborhood_tokens",
           "PretrainVisionTransformerEncoder", "PretrainVisionTransformerDecoder", "PretrainVisionTransformer", "mae_reconstruction_loss",
           "KaldiFbank", "ASTModel", "mel_filterbank", "fbank_tables", "specaug_bands"]
