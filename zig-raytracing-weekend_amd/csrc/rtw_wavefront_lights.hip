// The wavefront kernels of contexts with registered lights (rtw_scene_set_lights: the RTW_F_ALL | RTW_F_PDF and
// RTW_F_ALL | RTW_F_TREE | RTW_F_PDF instantiations of every kernel family an RTW_F_ALL scene can reach) as their
// own translation unit: they compile beside rtw_wavefront.hip instead of after it, and the kernels of contexts
// without lights are built from exactly the instantiations they were (DESIGN.md §light sampling).
#define RTW_WF_LIGHTS_TU
#include "rtw_wavefront.hip"
