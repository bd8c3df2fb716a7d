"""Host restatement of the depth-image tail of adapt_multitask_tester.py:148-155 (transform.py:285-294, ``unnormalize``): the rule
``mcdseg_depth_image_u8`` implements, written out in numpy without calling numpy's own float -> uint8 cast."""
import numpy as np

MEAN = np.array([.485, .456, .406])  # transform.py:287-288 (not the training transform's statistics)
STD = np.array([.229, .224, .225])


def numpy_u8(t):
    """np.uint8(t) of a float64 array on x86-64: truncate toward zero to int32 and keep the low 8 bits; NaN, +-inf and values
    outside the int32 range give 0."""
    t = np.asarray(t, dtype=np.float64)
    ok = (t > -2147483649.0) & (t < 2147483648.0)  # False for NaN
    return np.where(ok, np.trunc(np.where(ok, t, 0.0)).astype(np.int64) & 255, 0).astype(np.uint8)


def unnormalize_u8(hwc):
    """float32 [..., H, W, Cd] (Cd = 1 or 3) -> uint8 [..., H, W, 3]: (v * STD + MEAN) * 255 in float64, each operation rounded
    (numpy's promotion of the float32 map against the float64 constants), Cd = 1 broadcast into three channels"""
    return numpy_u8(((np.asarray(hwc, dtype=np.float32).astype(np.float64) * STD) + MEAN) * 255.0)
