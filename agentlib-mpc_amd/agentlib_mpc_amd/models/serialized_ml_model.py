"""Serialized data-driven models (the ``ml_model_sources`` of a ``CasadiMLModel``).

Restates `agentlib_mpc/models/serialized_ml_model.py`: the pydantic container
``SerializedMLModel`` (:30-153: ``dt``, ``input``, ``output``,
``training_info``, ``model_type``; loading from a dict, JSON string or file)
and ``SerializedANN`` (:155-228: ``structure`` = the keras model JSON,
``weights`` = per-layer lists of arrays).  Keras is not part of this
framework: the ANN structure JSON is read directly (layer ``class_name`` and
``config``), which is all the CasADi translation of the reference uses
(`models/casadi_predictor.py:306-376`).

``SerializedGPR`` (:410-540) and ``SerializedLinReg`` (:566-659) carry the
fitted parameters of a scikit-learn ``GaussianProcessRegressor``
(``ConstantKernel * RBF + WhiteKernel``) and ``LinearRegression`` with the
reference's field names, defaults and JSON layout, so a file written by the
reference's ``save_serialized_model`` loads unchanged.  Only the fields the
posterior mean needs are used (``alpha``, ``X_train``, ``constant_value``,
``length_scale``, ``data_handling``; ``coef``, ``intercept``); ``L``,
``y_train``, the bounds and ``theta`` are kept for round trips.  scikit-learn
is no dependency of the package: ``serialize`` imports it inside the function
and reads the fitted attributes of the estimator it is handed; ``deserialize``
and the trainers are out of scope.  ``KerasANN`` models are not supported.
"""

from __future__ import annotations

import json
from enum import Enum
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np
from pydantic import BaseModel, ConfigDict, Field, model_validator

from agentlib_mpc_amd.data_structures.ml_model_datatypes import Feature, OutputFeature, column_order


class MLModels(str, Enum):
    ANN = "ANN"
    GPR = "GPR"
    LINREG = "LinReg"
    KerasANN = "KerasANN"


class SerializedMLModel(BaseModel):
    dt: Union[float, int] = Field(title="dt", description="Length of one prediction step in seconds.")
    input: Dict[str, Feature] = Field(default=None, title="input")
    output: Dict[str, OutputFeature] = Field(default=None, title="output")
    training_info: Optional[dict] = Field(default=None, title="Training Info")
    model_type: MLModels
    model_config = ConfigDict(protected_namespaces=(), extra="allow")

    @classmethod
    def load_serialized_model_from_dict(cls, model_data: dict) -> "SerializedMLModel":
        model_type = model_data.get("model_type")
        if model_type in (MLModels.ANN, MLModels.ANN.value):
            return SerializedANN(**model_data)
        if model_type in (MLModels.GPR, MLModels.GPR.value):
            return SerializedGPR(**model_data)
        if model_type in (MLModels.LINREG, MLModels.LINREG.value):
            return SerializedLinReg(**model_data)
        raise NotImplementedError(
            f"ML model type {model_type!r} is not supported by the MI355X backend (ANN, GPR and LinReg only).")

    @classmethod
    def load_serialized_model_from_string(cls, json_string: str) -> "SerializedMLModel":
        return cls.load_serialized_model_from_dict(json.loads(json_string))

    @classmethod
    def load_serialized_model_from_file(cls, path: Path) -> "SerializedMLModel":
        with open(path, "r") as f:
            return cls.load_serialized_model_from_dict(json.load(f))

    @classmethod
    def load_serialized_model(cls, model_data: Union[dict, str, Path]) -> "SerializedMLModel":
        if isinstance(model_data, dict):
            return cls.load_serialized_model_from_dict(model_data)
        if isinstance(model_data, (str, Path)) and Path(model_data).exists():
            return cls.load_serialized_model_from_file(Path(model_data))
        return cls.load_serialized_model_from_string(str(model_data))

    def save_serialized_model(self, path: Path):
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        with open(path, "w") as f:
            f.write(self.model_dump_json())


class SerializedANN(SerializedMLModel):
    """Keras-structure JSON + per-layer weight lists (`serialized_ml_model.py:155-228`)."""

    weights: List[list] = Field(default=None, title="weights")
    structure: str = Field(default=None, title="structure")
    model_type: MLModels = MLModels.ANN

    def layer_specs(self) -> List[dict]:
        """Layers with their weights as numpy arrays: ``[{"class_name", "config", "weights"}]``.

        ``InputLayer`` entries of the structure carry no weights and are skipped,
        matching keras' ``model.layers`` (which the weights list was taken from).
        """
        struct = json.loads(self.structure)
        cfg = struct.get("config", {})
        layers = cfg.get("layers", cfg if isinstance(cfg, list) else [])
        layers = [l for l in layers if l.get("class_name") != "InputLayer"]
        if len(layers) != len(self.weights):
            raise ValueError(f"ANN structure has {len(layers)} layers but {len(self.weights)} weight lists")
        return [{"class_name": l["class_name"], "config": l.get("config", {}),
                 "weights": [np.asarray(w, dtype=float) for w in ws]}
                for l, ws in zip(layers, self.weights)]

    @classmethod
    def from_layers(cls, layers: List[dict], dt, input: Dict[str, Feature],
                    output: Dict[str, OutputFeature], training_info: Optional[dict] = None
                    ) -> "SerializedANN":
        """Build from ``[{"class_name", "config", "weights": [arrays]}]`` (keras-equivalent
        structure JSON), e.g. for synthetic networks."""
        structure = json.dumps({"class_name": "Sequential", "config": {
            "name": "sequential", "layers": [{"class_name": l["class_name"], "config": l.get("config", {})}
                                             for l in layers]}})
        weights = [[np.asarray(w, dtype=float).tolist() for w in l["weights"]] for l in layers]
        return cls(structure=structure, weights=weights, dt=dt, input=input, output=output,
                   training_info=training_info)


def _n_columns(model: SerializedMLModel) -> Optional[int]:
    """Number of lagged input columns, or None while the features are not set."""
    if model.input is None or model.output is None:
        return None
    return len(column_order(model.input, model.output))


class GPRDataHandlingParameters(BaseModel):
    """Input normalisation and output scaling of a GPR (`serialized_ml_model.py:231-251`)."""

    normalize: bool = Field(default=False, title="normalize",
                            description="Whether the inputs are normalised with mean and std.")
    scale: float = Field(default=1.0, title="scale",
                         description="Factor applied to the prediction (y was divided by it for the fit).")
    mean: Optional[list] = Field(default=None, title="mean", description="Per-input mean (normalize only).")
    std: Optional[list] = Field(default=None, title="standard deviation",
                                description="Per-input standard deviation (normalize only).")


class GPRKernelParameters(BaseModel):
    """``ConstantKernel * RBF + WhiteKernel`` of the fitted GPR (`serialized_ml_model.py:304-357`)."""

    constant_value: float = Field(default=1.0, title="constant value")
    constant_value_bounds: Union[tuple, str] = Field(default=(1e-5, 1e5), title="constant value bounds")
    length_scale: Union[float, list] = Field(default=1.0, title="length_scale",
                                             description="Scalar (isotropic) or one entry per input.")
    length_scale_bounds: Union[tuple, str] = Field(default=(1e-5, 1e5), title="length_scale_bounds")
    noise_level: float = Field(default=1.0, title="noise level",
                               description="WhiteKernel variance; takes no part in the mean.")
    noise_level_bounds: Union[tuple, str] = Field(default=(1e-5, 1e5), title="noise level bounds")
    theta: list = Field(title="theta", description="Log-transformed free kernel parameters (kept, not used).")
    model_config = ConfigDict(arbitrary_types_allowed=True)

    @classmethod
    def from_model(cls, model) -> "GPRKernelParameters":
        rbf, const, white = model.kernel_.k1.k2, model.kernel_.k1.k1, model.kernel_.k2
        ls = np.asarray(rbf.length_scale, dtype=float)
        return cls(constant_value=float(const.constant_value), constant_value_bounds=_bounds(const.constant_value_bounds),
                   length_scale=float(ls) if ls.ndim == 0 else ls.tolist(),
                   length_scale_bounds=_bounds(rbf.length_scale_bounds), noise_level=float(white.noise_level),
                   noise_level_bounds=_bounds(white.noise_level_bounds), theta=np.asarray(model.kernel_.theta).tolist())


def _bounds(b):
    return b if isinstance(b, str) else tuple(np.asarray(b, dtype=float).reshape(-1).tolist())


class GPRParameters(BaseModel):
    """Fitted data of the GPR (`serialized_ml_model.py:360-407`)."""

    alpha: Union[float, list] = Field(default=1e-10, title="alpha",
                                      description="Dual coefficients of the training points, [NT] or [NT, n_out].")
    L: list = Field(title="L", description="Cholesky factor of the training kernel (kept, not used).")
    X_train: list = Field(title="X_train", description="Training points [NT, n_features_in].")
    y_train: list = Field(title="y_train", description="Training targets (kept, not used).")
    n_features_in: int = Field(title="number of input features")
    log_marginal_likelihood_value: float = Field(title="log marginal likelihood value")
    model_config = ConfigDict(arbitrary_types_allowed=True)

    @classmethod
    def from_model(cls, model) -> "GPRParameters":
        return cls(alpha=np.asarray(model.alpha_).tolist(), L=np.asarray(model.L_).tolist(),
                   X_train=np.asarray(model.X_train_).tolist(), y_train=np.asarray(model.y_train_).tolist(),
                   n_features_in=int(model.n_features_in_),
                   log_marginal_likelihood_value=float(model.log_marginal_likelihood_value_))


class SerializedGPR(SerializedMLModel):
    """Posterior mean of a fitted Gaussian process (`serialized_ml_model.py:410-477`)."""

    data_handling: GPRDataHandlingParameters = Field(default=None, title="data_handling")
    kernel_parameters: GPRKernelParameters = Field(default=None, title="kernel parameters")
    gpr_parameters: GPRParameters = Field(default=None, title="gpr_parameters")
    model_config = ConfigDict(arbitrary_types_allowed=True, protected_namespaces=(), extra="allow")
    model_type: MLModels = MLModels.GPR

    @model_validator(mode="after")
    def _shapes_agree(self):
        gp, kp, dh = self.gpr_parameters, self.kernel_parameters, self.data_handling
        if gp is None:
            return self
        X = np.asarray(gp.X_train, dtype=float)
        if X.ndim != 2 or X.shape[1] != gp.n_features_in:
            raise ValueError(f"X_train has shape {X.shape}, but n_features_in is {gp.n_features_in}")
        ncol = _n_columns(self)
        if ncol is not None and ncol != gp.n_features_in:
            raise ValueError(f"n_features_in is {gp.n_features_in}, but input and output define {ncol} lagged columns")
        alpha = np.asarray(gp.alpha, dtype=float)
        n_out = 1 if self.output is None else len(self.output)
        if alpha.ndim not in (1, 2) or alpha.shape[0] != X.shape[0] or (alpha.shape[1] if alpha.ndim == 2 else 1) != n_out:
            raise ValueError(f"alpha has shape {alpha.shape}, expected [{X.shape[0]}] or [{X.shape[0]}, n_out] "
                             f"for {n_out} output(s)")
        if kp is not None:
            ls = np.asarray(kp.length_scale, dtype=float)
            if ls.ndim > 1 or (ls.ndim == 1 and ls.shape[0] != gp.n_features_in):
                raise ValueError(f"length_scale has shape {ls.shape}, expected a scalar or [{gp.n_features_in}]")
        if dh is not None and dh.normalize:
            if dh.mean is None or dh.std is None:
                raise ValueError("Mean and std are not valid: data_handling.mean and data_handling.std are needed "
                                 "when normalize is true.")
            for name, v in (("mean", dh.mean), ("std", dh.std)):
                if len(v) != gp.n_features_in:
                    raise ValueError(f"data_handling.{name} has {len(v)} entries, expected {gp.n_features_in}")
        return self

    @classmethod
    def serialize(cls, model, dt: Union[float, int], input: Dict[str, Feature], output: Dict[str, OutputFeature],
                  training_info: Optional[dict] = None) -> "SerializedGPR":
        """From a fitted scikit-learn ``GaussianProcessRegressor`` with the kernel
        ``ConstantKernel * RBF + WhiteKernel``; its optional ``data_handling`` attribute (the
        reference's ``CustomGPR``) carries the normalisation."""
        from sklearn.gaussian_process import GaussianProcessRegressor  # noqa: F401  (not a package dependency)

        if not all(hasattr(model, attr) for attr in ["kernel_", "alpha_", "L_", "X_train_", "y_train_"]):
            raise ValueError("To serialize a GPR, a fitted GPR must be passed, "
                             "but an unfitted GPR has been passed here.")
        dh = getattr(model, "data_handling", None)
        if dh is None:
            dh = GPRDataHandlingParameters()
        elif not isinstance(dh, (dict, GPRDataHandlingParameters)):
            dh = {k: getattr(dh, k) for k in ("normalize", "scale", "mean", "std")}
        if isinstance(dh, dict):
            dh = GPRDataHandlingParameters(**{k: (np.asarray(v).tolist() if k in ("mean", "std") and v is not None else v)
                                              for k, v in dh.items()})
        return cls(dt=dt, input=input, output=output, data_handling=dh,
                   kernel_parameters=GPRKernelParameters.from_model(model),
                   gpr_parameters=GPRParameters.from_model(model), trainer_config=training_info)


class LinRegParameters(BaseModel):
    """Fitted ``LinearRegression`` (`serialized_ml_model.py:543-563`)."""

    coef: list = Field(title="coefficients", description="[n_targets, n_features], or [n_features] for one target.")
    intercept: Union[float, list] = Field(title="intercept")
    n_features_in: int = Field(title="number of input features")
    rank: int = Field(title="rank", description="Rank of the training matrix (kept, not used).")
    singular: list = Field(title="singular", description="Its singular values (kept, not used).")


class SerializedLinReg(SerializedMLModel):
    """``intercept + x @ coef.T`` (`serialized_ml_model.py:566-626`)."""

    parameters: LinRegParameters = Field(title="parameters")
    model_config = ConfigDict(arbitrary_types_allowed=True, protected_namespaces=(), extra="allow")
    model_type: MLModels = MLModels.LINREG

    @model_validator(mode="after")
    def _shapes_agree(self):
        par = self.parameters
        coef = np.asarray(par.coef, dtype=float)
        n_out = 1 if self.output is None else len(self.output)
        ok = (coef.ndim == 1 and n_out == 1 and coef.shape[0] == par.n_features_in) or \
             (coef.ndim == 2 and coef.shape == (n_out, par.n_features_in))
        if not ok:
            raise ValueError(f"coef has shape {coef.shape}, expected [{n_out}, {par.n_features_in}]"
                             f"{' or [%d]' % par.n_features_in if n_out == 1 else ''}")
        ncol = _n_columns(self)
        if ncol is not None and ncol != par.n_features_in:
            raise ValueError(f"n_features_in is {par.n_features_in}, but input and output define {ncol} lagged columns")
        if np.asarray(par.intercept, dtype=float).size not in (1, n_out):
            raise ValueError(f"intercept has {np.asarray(par.intercept).size} entries, expected {n_out}")
        return self

    @classmethod
    def serialize(cls, model, dt: Union[float, int], input: Dict[str, Feature], output: Dict[str, OutputFeature],
                  training_info: Optional[dict] = None) -> "SerializedLinReg":
        """From a fitted scikit-learn ``LinearRegression``."""
        from sklearn.linear_model import LinearRegression  # noqa: F401  (not a package dependency)

        if not all(hasattr(model, attr) for attr in ["coef_", "intercept_", "n_features_in_", "rank_", "singular_"]):
            raise ValueError("To serialize a GPR, a fitted GPR must be passed, "
                             "but an unfitted GPR has been passed here.")
        parameters = LinRegParameters(coef=np.asarray(model.coef_).tolist(),
                                      intercept=np.asarray(model.intercept_).tolist(),
                                      n_features_in=int(model.n_features_in_), rank=int(model.rank_),
                                      singular=np.asarray(model.singular_).tolist())
        return cls(dt=dt, input=input, output=output, parameters=parameters, trainer_config=training_info)
