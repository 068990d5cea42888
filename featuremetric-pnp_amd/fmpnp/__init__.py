"""fmpnp -- MI355X-native feature-metric PnP refiner (drop-in for aunagar/FeatureMetric-PnP's
sparseFeaturePnP / feature_pnp / optimize_feature_pnp).  The compute path is libfmpnp.so
(HIP, gfx950); there is no CPU fallback."""
from . import _lib, config, losses, refine  # noqa: F401
from .losses import (barron, barron_loss, cauchy_loss, geman_mcclure_loss, huber_loss, scaled_loss,  # noqa: F401
                     squared_loss)
from .matrix_utils import matrix_quaternion  # noqa: F401
from .model import find_inliers, sparseFeaturePnP  # noqa: F401
from .optimize_feature_pnp import DirectPoseModel, feature_pnp, feature_pnp_multi, optimize_feature_pnp  # noqa: F401
from .refine import AsyncBatch, PackedFeatures, Problem, make_options, make_problem, pack_features  # noqa: F401
from . import cpu, pipeline, replay  # noqa: F401,E402
from .pipeline import RefinePipeline  # noqa: F401,E402
from . import match  # noqa: F401,E402
from .match import (exhaustive_match, exhaustive_match_cpu, exhaustive_search, exhaustive_search_multi,  # noqa: F401,E402
                    exhaustive_match_layers, exhaustive_match_layers_cpu, exhaustive_search_layers,
                    exhaustive_search_layers_multi, fast_sparse_keypoint_descriptor, gather_sparse_descriptors,
                    generate_dense_keypoints, nearest_cells)
from . import pnp  # noqa: F401,E402
from .pnp import Prediction, solve_pnp, solve_pnp_multi  # noqa: F401,E402
from . import hypercolumn  # noqa: F401,E402
from .hypercolumn import (HypercolumnExtractor, assemble_hypercolumn, assemble_hypercolumn_cpu,  # noqa: F401,E402
                          pack_hypercolumn, pack_hypercolumn_cpu, sparse_hypercolumn, sparse_hypercolumn_cpu)
from . import retrieval  # noqa: F401,E402
from .retrieval import (NetVLAD, compute_embedding, compute_ranks, learn_and_apply_pca, netvlad_pool,  # noqa: F401,E402
                        netvlad_pool_cpu, rank_topn, rank_topn_cpu)
from . import localize as _localize  # noqa: F401,E402
from .localize import Localization, LocalizeLaunch, localize, localize_cpu, localize_multi  # noqa: F401,E402
from . import superpoint  # noqa: F401,E402
from .superpoint import (HipSuperPointNet, SuperPointFrontend, SuperPointNet, assemble_matches, fast_closest_points,  # noqa: F401,E402
                         fast_keypoint_matching, superpoint_localize, superpoint_postprocess)
from . import encoder  # noqa: F401,E402
from .encoder import (HipEncoder, avgpool2x2s1, avgpool2x2s1_cpu, conv1x1, conv1x1_cpu, conv3x3, conv3x3_cpu,  # noqa: F401,E402
                      conv3x3_f16_weights, maxpool2x2, maxpool2x2_cpu, relu, relu_cpu)
from . import dense  # noqa: F401,E402
from .dense import (DenseFeatureExtractor, d2net_preprocess, d2net_trunk, dense_pyramid_step,  # noqa: F401,E402
                    dense_pyramid_step_cpu)
from . import image  # noqa: F401,E402
from .image import (image_loader, image_to_tensor, image_to_tensor_cpu, load_images, resize_lanczos,  # noqa: F401,E402
                    resize_lanczos_cpu, superpoint_image, thumbnail_size)

__version__ = "0.1.0"
