"""Heat maps and landmarks of an image batch (reference Util/landmark_util.py:19-255), with the reference's names.

The two networks are the caller's: `fa` is a face_alignment.FaceAlignment (or anything with its two attributes),
    fa.face_detector.face_detector    the SFD detector network: image batch -> list of class / regression maps
    fa.face_detector._filter_bboxes, .reference_scale
    fa.face_alignment_net             the FAN: [N, 3, 256, 256] crops in [0, 1] -> [N, 68, 64, 64] heat maps
Everything between them is tensor work and runs on this package's kernels (op/landmark.py, csrc/landmark.hip): the
detector's input in one launch, every crop of the batch in one launch (forward and backward), the decode of all heat maps
in one launch.  The only host copy is the detector's output (one tensor); after it nothing synchronises.

What is different, on purpose:
  * the detector runs under no_grad: its outputs only ever leave as host data (`.data.cpu()`), the reference builds a graph
    it never uses;
  * `transform` is written out here (the third-party package's formula, float32); the boxes of the crops are computed with it
    on the host, where the box list is anyway, and the decode kernel uses its closed-form inverse;
  * `get_predictions` (box decoding of the detector's maps) stays the package's: it is imported from the installed
    `face_alignment` when Batch_Img_Face_Detection is called, which raises ImportError naming the package without it;
  * Get_HeatMap_Landmark_PyTorch decodes on the device with Get_Preds_FromHeatMap_PyTorch and returns a tensor: the
    reference's numpy `get_preds_fromhm` is the package's (its sub-pixel step and rounding differ between releases) and
    cannot be pinned here;
  * images and crops may have any size; `resolution` (256) is the crop's.
"""
import torch
import torch.nn.functional as F

from op import landmark as L

RESOLUTION = 256                 # side of the alignment network's input (Crop_PyTorch's default)
FALLBACK_BBOX = [0, 0, 255, 255, 1]


def transform(point, center, scale, resolution, invert=False):
    """The package's point transform in float32: with h = 200 * scale and r = resolution,
    t = [[r/h, 0, r(-cx/h + 1/2)], [0, r/h, r(-cy/h + 1/2)], [0, 0, 1]], inverted when `invert`; returns
    (t . [x, y, 1])[:2] as an int32 tensor (truncation toward zero)."""
    pt = torch.ones(3)
    pt[0], pt[1] = float(point[0]), float(point[1])
    h = 200.0 * torch.as_tensor(scale, dtype=torch.float32)
    center = torch.as_tensor(center, dtype=torch.float32)
    t = torch.eye(3)
    t[0, 0] = resolution / h
    t[1, 1] = resolution / h
    t[0, 2] = resolution * (-center[0] / h + 0.5)
    t[1, 2] = resolution * (-center[1] / h + 0.5)
    if invert:
        t = torch.inverse(t)
    return torch.matmul(t, pt)[0:2].int()


def _get_predictions():
    try:
        from face_alignment.detection.sfd.detect import get_predictions
    except ImportError as e:
        raise ImportError('Batch_Img_Face_Detection decodes the detector\'s maps with get_predictions of the '
                          '`face_alignment` package (face_alignment.detection.sfd.detect), which is not installed') from e
    return get_predictions


def Batch_Img_Face_Detection(img_tensor, face_detector, device, scaled=True):
    """One bounding box [x0, y0, x1, y1, score] per image of a batch of single-face images (landmark_util.py:19-51).
    img_tensor [N, 3, H, W]: in [0, 255] as in the reference (scaled=True), or in [-1, 1] (scaled=False: the scaling, the
    channel flip and the mean subtraction are then one launch).  face_detector: the SFDDetector (its .face_detector
    network, ._filter_bboxes).  A batch whose image has no box, or whose first box leaves [0, 255], gets the reference's
    fallback [0, 0, 255, 255, 1]."""
    get_predictions = _get_predictions()
    with torch.no_grad():
        if scaled:
            mean = torch.tensor(L.DETECTOR_MEAN, device=img_tensor.device, dtype=img_tensor.dtype).view(1, 3, 1, 1)
            img = img_tensor.flip(-3) - mean
        else:
            img = L.detector_input(img_tensor)
        olist = list(face_detector.face_detector(img))
        for i in range(len(olist) // 2):
            olist[i * 2] = F.softmax(olist[i * 2], dim=1)
        # one host copy for all maps
        shapes = [tuple(o.shape) for o in olist]
        flat = torch.cat([o.detach().reshape(-1).to(torch.float32) for o in olist]).cpu().numpy()
    maps, start = [], 0
    for s in shapes:
        n = 1
        for d in s:
            n *= d
        maps.append(flat[start:start + n].reshape(s))
        start += n
    bbox_list = []
    for i in range(img.shape[0]):
        bboxlists = get_predictions([m[i:i + 1, ...] for m in maps], 1)[0]
        bboxlists = face_detector._filter_bboxes(bboxlists)
        if len(bboxlists) == 0:
            bbox_list.append(list(FALLBACK_BBOX))
        elif (bboxlists[0][0] < 0) or (bboxlists[0][1] < 0) or (bboxlists[0][2] > 255) or (bboxlists[0][3] > 255):
            bbox_list.append(list(FALLBACK_BBOX))
        else:
            bbox_list.append(bboxlists[0])
    return bbox_list


def Box_Center_Scale(bbox, reference_scale):
    """(center, scale) of a bounding box (landmark_util.py:96-98): the centre of the box, shifted up by 0.12 of its
    height, as a float32 tensor of two, and scale = (width + height) / reference_scale."""
    center = torch.tensor([bbox[2] - (bbox[2] - bbox[0]) / 2.0, bbox[3] - (bbox[3] - bbox[1]) / 2.0])
    center[1] = center[1] - (bbox[3] - bbox[1]) * 0.12
    scale = (bbox[2] - bbox[0] + bbox[3] - bbox[1]) / reference_scale
    return center, scale


def Face_Crop_Boxes(center_list, scale_list, resolution=RESOLUTION):
    """[N, 4] int32 host tensor (ux, uy, bx, by): per sample the inverse transform of (1, 1) and of (resolution,
    resolution), the corners Crop_PyTorch cuts (landmark_util.py:64-65)."""
    rows = []
    for center, scale in zip(center_list, scale_list):
        ul = transform([1, 1], center, scale, resolution, True)
        br = transform([resolution, resolution], center, scale, resolution, True)
        rows.append(torch.stack((ul[0], ul[1], br[0], br[1])))
    return torch.stack(rows).to(torch.int32)


def Crop_An_Image(img_tensor, bbox, reference_scale, resolution=RESOLUTION):
    """(crop, center, scale) of one image [1, 3, H, W] in [0, 255] around a bounding box (landmark_util.py:85-101): the
    crop [1, 3, resolution, resolution] keeps the image's range.  The batch path is Get_HeatMap_PyTorch's one launch; this
    single-image form evaluates the composite on the image's device."""
    center, scale = Box_Center_Scale(bbox, reference_scale)
    box = Face_Crop_Boxes([center], [scale], resolution)
    return L.crop_canvas(img_tensor, box, resolution), center, scale


def Get_Preds_FromHeatMap_PyTorch(hm, device=None, center_list=None, scale_list=None):
    """(preds, preds_orig), each [B, C, 2], of heat maps hm [B, C, 64, 64] (landmark_util.py:105-164): the maxima in
    map coordinates, and in the image's frame when center_list and scale_list are given (zeros otherwise).  One launch
    for all B * C maps; `device` is kept for the reference's signature."""
    return L.landmark_decode(hm, center_list, scale_list)


def Get_HeatMap_PyTorch(img_tensor, fa, device=None, resolution=RESOLUTION):
    """(heatmap, center_list, scale_list) of img_tensor [N, 3, H, W] in [-1, 1] (landmark_util.py:169-201): detection,
    one crop launch for the batch, the alignment network.  Differentiable with respect to img_tensor through the crop."""
    bbox_list = Batch_Img_Face_Detection(img_tensor, fa.face_detector, device, scaled=False)
    center_list, scale_list = [], []
    for bbox in bbox_list:
        center, scale = Box_Center_Scale(bbox, fa.face_detector.reference_scale)
        center_list.append(center)
        scale_list.append(scale)
    box = Face_Crop_Boxes(center_list, scale_list, resolution)
    heatmap = fa.face_alignment_net(L.face_crop(img_tensor, box, resolution))
    return heatmap, center_list, scale_list


def Get_HeatMap_Landmark_PyTorch(img_tensor, fa, device=None):
    """(heatmap [N, 68, 64, 64], landmark [N, 68, 2]) (landmark_util.py:204-233).  The landmarks come from the device
    decode (Get_Preds_FromHeatMap_PyTorch's preds_orig, a tensor on the heat maps' device): the reference calls the
    package's numpy get_preds_fromhm here, which is not part of this build and cannot be pinned."""
    heatmap, center_list, scale_list = Get_HeatMap_PyTorch(img_tensor, fa, device)
    _, landmark = Get_Preds_FromHeatMap_PyTorch(heatmap, device, center_list, scale_list)
    return heatmap, landmark


def Get_Landmark_PyTorch(img_tensor, fa, device=None):
    """landmark [N, 68, 2] in the image's frame (landmark_util.py:236-255)."""
    return Get_HeatMap_Landmark_PyTorch(img_tensor, fa, device)[1]
