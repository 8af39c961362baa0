"""Detector models -- drop-in for reference skyeye/core/models/detector.py.

Same classes, constructor arguments, attributes (``cfg``, ``stride``, ``names``, ``backbone``, ``neck``,
``detection_head``) and return values; the forward pass is the MI355X engine.  The reference's own
``SkyEyeDetector`` cannot be constructed or run; the wiring fixes adopted here are
  D1  the neck is built with width scale 1 on the backbone's already-scaled channels (detector.py:165-166,276-279)
  D2  neck / head widths come from the backbone's real feature channels (backbone.py:139-143 vs :40-42,99)
  D3  ``_initialize_weights`` skips the missing bias of ``nn.Linear(bias=False)`` (detector.py:339-341)
  D4  EnhancedSkyEyeDetector's cross-layer attention projects key/value to the query width (detector.py:457-469)
"""
import math
import os
from pathlib import Path

import torch
import torch.nn as nn
import yaml

from ._base import BatchNormParams, Conv2dParams, LinearParams, NativeModule
from .attention import CrossLayerAttention
from .backbone import SkyEyeBackbone
from .blocks import ConvolutionBlock, CSPBlock, SPPBlock  # noqa: F401  (re-exported like the reference)

DEFAULT_ANCHORS = [[[10, 13], [16, 30], [33, 23]], [[30, 61], [62, 45], [59, 119]], [[116, 90], [156, 198], [373, 326]]]


class DetectionHead(NativeModule):
    """1x1 prediction convs + box decoding  (reference detector.py:18-145)."""
    _sky_module = "HEAD"

    def __init__(self, num_classes=80, anchors=None, channels=None):
        super().__init__()
        self.num_classes = num_classes
        self.num_outputs = num_classes + 5
        self.anchors = anchors if anchors is not None else DEFAULT_ANCHORS
        self.num_anchors = len(self.anchors[0]) if self.anchors else 3
        self.num_layers = len(self.anchors) if self.anchors else 3
        self.grid = [torch.zeros(1)] * self.num_layers
        self.anchor_grid = [torch.zeros(1)] * self.num_layers
        if channels is None:
            channels = [256, 512, 1024]
        self.channels = list(channels)
        self.detection_layers = nn.ModuleList(Conv2dParams(ch, self.num_anchors * self.num_outputs, 1, bias=True) for ch in channels)

    def _sky_config(self):
        return dict(nc=self.num_classes, anchors=self.anchors, level_channels=self.channels, input_h=0, input_w=0)

    def forward(self, feature_maps):
        """-> list of raw [B, anchors, H, W, outputs] tensors (detector.py:61-86)."""
        # the decoded tensor the engine also produces is discarded here; strides need a nominal input size
        gh, gw = feature_maps[0].shape[2:]
        outs = self._run(list(feature_maps), dict(input_h=int(gh) * 8, input_w=int(gw) * 8))
        return outs[1:]

    def process_detections(self, outputs, input_shape):
        """raw levels -> [B, sum(anchors*H*W), outputs] boxes (detector.py:88-145); anchor*stride quirk (D13) kept."""
        dec = _Decode(self.num_classes, self.anchors)
        # same engine as the head itself: the bf16 engine's decode uses the fast sigmoid of its fused epilogue, the exact
        # engine the IEEE one, so that detect() and forward() + process_detections() agree bit for bit
        dec.__dict__["_precision"] = self._resolved_precision()
        return dec._run(list(outputs), dict(input_h=int(input_shape[0]), input_w=int(input_shape[1])))[0]

    def detect(self, feature_maps, input_shape):
        """forward + process_detections in one engine call -> (detections, raw outputs)."""
        outs = self._run(list(feature_maps), dict(input_h=int(input_shape[0]), input_w=int(input_shape[1])))
        return outs[0], outs[1:]


class _Decode(NativeModule):
    _sky_module = "DECODE"

    def __init__(self, num_classes, anchors):
        super().__init__()
        self._cfg = dict(nc=num_classes, anchors=anchors)

    def _sky_config(self):
        return self._cfg


class FeatureNeck(NativeModule):
    """Top-down + bottom-up fusion  (reference detector.py:148-231)."""
    _sky_module = "NECK"

    def __init__(self, in_channels, width_multiple=1.0):
        super().__init__()

        def scaled_channels(x):
            return max(round(x * width_multiple), 1)

        if width_multiple != 1.0:
            raise NotImplementedError("FeatureNeck re-applies width_multiple to already scaled channels in the reference "
                                      "(detector.py:165-166); only width_multiple=1.0 yields a consistent graph (SURVEY D1)")
        c3, c4, c5 = in_channels
        self.lateral_conv5 = ConvolutionBlock(c5, scaled_channels(c4), 1, 1)
        self.lateral_conv4 = ConvolutionBlock(c4, scaled_channels(c3), 1, 1)
        self.fpn_conv4 = CSPBlock(scaled_channels(c4) * 2, scaled_channels(c4), num_blocks=3)
        self.fpn_conv3 = CSPBlock(scaled_channels(c3) * 2, scaled_channels(c3), num_blocks=3)
        self.downsample3 = ConvolutionBlock(scaled_channels(c3), scaled_channels(c3), 3, 2)
        self.downsample4 = ConvolutionBlock(scaled_channels(c4), scaled_channels(c4), 3, 2)
        self.pan_conv4 = CSPBlock(scaled_channels(c3) + scaled_channels(c4), scaled_channels(c4), num_blocks=3)
        self.pan_conv5 = CSPBlock(scaled_channels(c4) + scaled_channels(c5), scaled_channels(c5), num_blocks=3)
        self.out_channels = [scaled_channels(c3), scaled_channels(c4), scaled_channels(c5)]
        self._cfg = dict(level_channels=[c3, c4, c5])

    def _sky_config(self):
        return self._cfg

    def forward(self, features):
        return self._run(list(features))


class SkyEyeDetector(NativeModule):
    """SkyEye detector  (reference detector.py:234-371)."""
    _sky_module = "DETECTOR"

    def __init__(self, cfg="skyeye_s.yaml", channels=3, num_classes=None, anchors=None, ch=None, nc=None):
        super().__init__()
        if ch is not None:          # spelling used by train.py:91
            channels = ch
        if nc is not None:
            num_classes = nc
        if isinstance(cfg, dict):
            self.cfg = cfg
        else:
            cfg_path = Path(cfg)
            if not cfg_path.exists():   # bare names resolve against the packaged configs
                cand = Path(__file__).resolve().parents[3] / "configs" / "models" / cfg_path.name
                if cand.exists():
                    cfg_path = cand
            with open(cfg_path, errors="ignore") as f:
                self.cfg = yaml.safe_load(f)
        if num_classes and num_classes != self.cfg["nc"]:
            self.cfg["nc"] = num_classes
        if anchors:
            self.cfg["anchors"] = anchors
        if channels != 3:
            raise NotImplementedError("FocusBlock(3, ...) is hard-wired in the reference backbone (backbone.py:48)")
        self.backbone = SkyEyeBackbone(base_channels=self.cfg.get("base_channels", 64),
                                       depth_multiple=self.cfg.get("depth_multiple", 1.0),
                                       width_multiple=self.cfg.get("width_multiple", 1.0))
        in_channels = self.backbone.channels                                     # D2: true channels
        self.neck = FeatureNeck(in_channels, width_multiple=1.0)                 # D1
        self.detection_head = DetectionHead(num_classes=self.cfg["nc"], anchors=self.cfg.get("anchors", None),
                                            channels=self.neck.out_channels)
        # optional YAML key `head_attention: true`: the reference's "transformer prediction heads" have no
        # call site; the build-defined wiring puts WindowedSelfAttention(window 8) on P3 / P4 and a TransformerLayer on P5
        # ahead of the detection convolutions.  H and W must then be multiples of 128 (P4 in whole windows).
        if self.cfg.get("head_attention", False):
            from .attention import TransformerLayer, WindowedSelfAttention
            c3, c4, c5 = self.neck.out_channels
            self.head_attention = nn.ModuleDict({"p3": WindowedSelfAttention(c3, 8, c3 // 32),
                                                 "p4": WindowedSelfAttention(c4, 8, c4 // 32),
                                                 "p5": TransformerLayer(c5, 8)})
        self._initialize_weights()
        # the reference discovers strides with a dry run on zeros(1, ch, 64, 64) (detector.py:274,291-295)
        self.stride = torch.tensor([8, 16, 32])
        self.names = [str(i) for i in range(self.cfg["nc"])]
        self.pt = True   # attribute read by detect.py:126

    def _sky_config(self):
        return dict(base_channels=self.cfg.get("base_channels", 64), depth_multiple=float(self.cfg.get("depth_multiple", 1.0)),
                    width_multiple=float(self.cfg.get("width_multiple", 1.0)), nc=self.cfg["nc"], in_channels=3,
                    anchors=self.detection_head.anchors, head_attention=bool(self.cfg.get("head_attention", False)))

    def forward(self, x, augment=False, visualize=False, return_raw=True):
        """eval: (detections [B, N, nc+5], [raw_P3, raw_P4, raw_P5]); train: raw list (detector.py:300-324).
        ``return_raw=False`` (eval only; an extension for callers that go straight to NMS, as validate.py:245-255 does): the
        engine skips the stores of the three raw levels (6 MB fp32 per 1280x1280 frame) and the second element is [].
        ``augment`` / ``visualize`` are accepted because the reference's callers pass them (validate.py:245, detect.py:140);
        ``augment=True`` (eval only) runs the 1 / 0.83-flipped / 0.67 schedule of ``skyeye.utils.tta.forward_augment`` and returns
        (detections [B, sum N_i, nc+5] in the frame of ``x``, None)."""
        if augment and not self.training:
            from ...utils.tta import forward_augment
            return forward_augment(lambda xi: self._run([xi])[0], x, gs=int(self.stride.max())), None
        if not self.training and not return_raw:
            return self._run([x], skip=(1, 2, 3))[0], []
        outs = self._run([x])
        if not self.training:
            return outs[0], outs[1:]
        return outs[1:]

    def detect_nms(self, x, conf_threshold=0.25, iou_threshold=0.45, max_detections=300, out=None, **nms_kw):
        """forward (raw levels not written) + non_max_suppression in one asynchronous call -> (rows [B, max_det, 7], counts [B]) on the
        device, the ``skyeye.utils.metrics.nms_raw`` result of ``self(x)[0]`` (validate.py:245-255 / detect.py:140-145 do exactly this
        pair).  An extension: with ``parallel_slices`` the NMS of a slice is enqueued on that slice's stream, so it runs beside the
        other slice's convolutions instead of behind the join.  ``out``: (rows, counts) to write into -- e.g. the views of a
        ``skyeye.distributed.BoxExchange`` block, so that the boxes land in the buffer the all-gather sends."""
        from ...utils.metrics import nms_raw
        if self.training:
            raise RuntimeError("detect_nms is an eval-mode call")
        xi = self._prepare_input(x)
        nsl = self.__dict__.get("_slices", 1)
        if nsl > 1 and self._sliceable([xi], nsl):
            B = xi.shape[0]
            cache = self._out_cache
            ck = ("nms", B, int(max_detections))
            bufs = out if out is not None else (cache.get(ck) if cache is not None else None)
            if bufs is None:
                bufs = (torch.empty((B, int(max_detections), 7), dtype=torch.float32, device=xi.device),
                        torch.empty((B,), dtype=torch.int32, device=xi.device))
                if cache is not None:
                    cache[ck] = bufs
            rows, counts = bufs

            def post(i, lo, hi, views):
                nms_raw(views[0], conf_threshold, iou_threshold, max_detections=max_detections, out=rows[lo:hi], counts=counts[lo:hi], **nms_kw)

            self._run_sliced([xi], None, (1, 2, 3), nsl, post=post)
            return rows, counts
        det = self._run([xi], skip=(1, 2, 3))[0]
        if out is not None:
            return nms_raw(det, conf_threshold, iou_threshold, max_detections=max_detections, out=out[0], counts=out[1], **nms_kw)
        return nms_raw(det, conf_threshold, iou_threshold, max_detections=max_detections, **nms_kw)

    def detect_nms_pipelined(self, x, conf_threshold=0.25, iou_threshold=0.45, max_detections=300, parity=None, out=None, **nms_kw):
        """A two-deep software pipeline over a stream of batches (an extension; validate.py:245-255 / detect.py:140-145 run the pair
        strictly one after the other): the forward pass of THIS batch is enqueued beside the non_max_suppression of the PREVIOUS one,
        which otherwise runs alone behind the join -- a chain of seven small kernels on a few CUs, 0.145 of 4.35 ms on the benchmark
        batch.  With ``parallel_slices`` that NMS runs on the last slice's stream behind the slice's forward pass, beside the other
        slices.  Returns (rows [B, max_det, 7], counts [B]) of the previous batch, or None for the first call; ``detect_nms_flush()``
        returns the last batch's.  Two sets of detection / NMS buffers alternate (``parity`` 0 / 1; given explicitly when the two
        forms are captured as two hipGraphs, else it toggles per call).  Needs ``reuse_output_buffers(True)``.  Same results as
        ``detect_nms`` on every batch (tests/test_gpu_slices.py).  ``out``: (rows, counts) for the PREVIOUS batch's boxes (the views of
        a ``BoxExchange`` block) instead of the module's own buffers."""
        from ...utils.metrics import nms_raw
        if self.training:
            raise RuntimeError("detect_nms_pipelined is an eval-mode call")
        if self._out_cache is None:
            raise RuntimeError("detect_nms_pipelined needs reuse_output_buffers(True): two batches are in flight")
        st = self.__dict__.setdefault("_pipe", {"parity": 0, "pending": None, "streams": {}})
        p = st["parity"] if parity is None else int(parity) & 1
        xi = self._prepare_input(x)
        dev = xi.device
        B = xi.shape[0]
        cur = torch.cuda.current_stream(dev)
        side = st["streams"].get(dev.index or 0)
        if side is None:
            # default priority: torch clamps a positive (lower-than-default) priority to 0, so no lower level is reachable through
            # torch.cuda.Stream -- round 3's "low-priority NMS stream, +0.9 %" was this same stream and run-to-run noise
            side = torch.cuda.Stream(device=dev)
            st["streams"][dev.index or 0] = side
        if parity is not None and st.get(("det", 1 - p)) is None:            # explicit parity (graph capture): the other set must exist
            self.__dict__["_out_slot"] = 2 - p
            try:
                st[("det", 1 - p)] = self._run([xi], skip=(1, 2, 3))[0]
            finally:
                self.__dict__["_out_slot"] = 0
        prev = st["pending"] if parity is None else st.get(("det", 1 - p))
        nsl = self.__dict__.get("_slices", 1)
        sliced = nsl > 1 and self._sliceable([xi], nsl)
        result, post, joined = None, None, False
        if prev is not None and prev.shape[0] != B:                            # batch size changed: the previous batch's NMS into fresh tensors
            result = nms_raw(prev, conf_threshold, iou_threshold, max_detections=max_detections, **nms_kw)
        elif prev is not None:
            ck = ("nms_pipe", B, int(max_detections), 1 - p)
            bufs = out if out is not None else self._out_cache.get(ck)
            if bufs is None:
                bufs = self._out_cache[ck] = (torch.empty((B, int(max_detections), 7), dtype=torch.float32, device=dev),
                                              torch.empty((B,), dtype=torch.int32, device=dev))
            if sliced:
                # on the last slice's stream behind that slice's forward pass, not on a stream of its own: captured, a third independent
                # chain beside the two slice chains gives a hipGraph whose replay segfaults in this runtime's hipGraphLaunch (graphs of two
                # independent chains, as detect_nms makes, replay)
                def post(i, lo, hi, views):
                    if i == nsl - 1:
                        nms_raw(prev, conf_threshold, iou_threshold, max_detections=max_detections, out=bufs[0], counts=bufs[1], **nms_kw)
            else:
                side.wait_stream(cur)                                          # fork: the previous batch's detections are complete on `cur`
                with torch.cuda.stream(side):
                    nms_raw(prev, conf_threshold, iou_threshold, max_detections=max_detections, out=bufs[0], counts=bufs[1], **nms_kw)
                joined = True
            result = bufs
        self.__dict__["_out_slot"] = 1 + p
        try:
            if sliced:
                det = self._run_sliced([xi], None, (1, 2, 3), nsl, post=post)[0]   # (the slice streams are joined into `cur` there)
            else:
                det = self._run([xi], skip=(1, 2, 3))[0]
        finally:
            self.__dict__["_out_slot"] = 0
        if joined:
            cur.wait_stream(side)                                              # join
        st[("det", p)] = det
        st["pending"] = det
        st["last"] = (p, conf_threshold, iou_threshold, int(max_detections), dict(nms_kw))
        if parity is None:
            st["parity"] = 1 - p
        return result

    def detect_nms_flush(self, parity=None):
        """non_max_suppression of the batch the last ``detect_nms_pipelined`` call ran forward: (rows, counts).  ``parity``: the set the
        last REPLAYED graph wrote, when the calls were captured."""
        from ...utils.metrics import nms_raw
        st = self.__dict__.get("_pipe")
        if not st or st.get("last") is None:
            raise RuntimeError("detect_nms_flush: nothing in flight")
        p, conf, iou, md, kw = st["last"]
        if parity is not None:
            p = int(parity) & 1
        return nms_raw(st[("det", p)], conf, iou, max_detections=md, **kw)

    def warmup(self, imgsz=(1, 3, 640, 640)):
        """detect.py:126 calls model.warmup(imgsz=...)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        self.forward(torch.zeros(*imgsz, device=dev))

    def _initialize_weights(self):
        """detector.py:326-341 with the D3 guard."""
        for m in self.modules():
            if isinstance(m, Conv2dParams):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, BatchNormParams):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, LinearParams):
                m.weight.data.normal_(0, 0.01)
                if m.bias is not None:
                    m.bias.data.zero_()
        self.refresh_weights()

    def load_from_pretrained(self, weights_path):
        """detector.py:343-371: accepts {'model': module}, {'state_dict': ...} or a bare state dict; keeps entries whose
        name and shape match.  torch >= 2.6 defaults to weights_only=True, which refuses pickled modules -- say so."""
        try:
            checkpoint = torch.load(weights_path, map_location="cpu", weights_only=True)
        except Exception as exc:  # noqa: BLE001
            raise RuntimeError(f"{weights_path}: not loadable with weights_only=True ({exc}); export a plain state dict") from exc
        if "model" in checkpoint and hasattr(checkpoint["model"], "state_dict"):
            state_dict = checkpoint["model"].float().state_dict()
        else:
            state_dict = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
        model_state_dict = self.state_dict()
        filtered = {k: v for k, v in state_dict.items() if k in model_state_dict and v.shape == model_state_dict[k].shape}
        self.load_state_dict(filtered, strict=False)
        print(f"Loaded {len(filtered)}/{len(model_state_dict)} layers from {weights_path}")
        return self


def parse_model(model_cfg, in_channels=3):
    """reference detector.py:374-406."""
    if isinstance(model_cfg, str):
        with open(model_cfg, errors="ignore") as f:
            cfg = yaml.safe_load(f)
    else:
        cfg = model_cfg
    return {"base_channels": cfg.get("base_channels", 64), "depth_multiple": cfg.get("depth_multiple", 1.0),
            "width_multiple": cfg.get("width_multiple", 1.0), "nc": cfg.get("nc", 80), "in_channels": in_channels,
            "anchors": cfg.get("anchors", None)}


def construct_model(model_cfg, in_channels=3, num_classes=None, anchors=None):
    """reference detector.py:409-433."""
    cfg = parse_model(model_cfg, in_channels)
    if num_classes is not None:
        cfg["nc"] = num_classes
    if anchors is not None:
        cfg["anchors"] = anchors
    return SkyEyeDetector(cfg, in_channels)


def load_model(weights, device=None, cfg="skyeye_s.yaml"):
    """Counterpart of the undefined ``load_model(weights, device)`` the reference CLIs import (validate.py:184)."""
    model = SkyEyeDetector(cfg)
    if weights:
        model.load_from_pretrained(weights)
    if device is not None:
        model.to(device)
    return model.eval()


class EnhancedSkyEyeDetector(SkyEyeDetector):
    """SkyEyeDetector + cross-layer attention between neck levels  (reference detector.py:436-501, with D4)."""
    _sky_module = "ENHANCED_DETECTOR"

    def __init__(self, cfg="skyeye_s.yaml", channels=3, num_classes=None, anchors=None):
        super().__init__(cfg, channels, num_classes, anchors)
        c3, c4, c5 = self.neck.out_channels
        self.cross_attention_p5_p4 = CrossLayerAttention(query_channels=c4, key_channels=c5, region_size=2, heads=4)
        self.cross_attention_p4_p3 = CrossLayerAttention(query_channels=c3, key_channels=c4, region_size=2, heads=4)
        self.refresh_weights()
