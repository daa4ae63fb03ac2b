// The wavefront kernels of contexts with registered vertex attributes (rtw_scene_set_vertex_attrs: the
// RTW_F_ALL | RTW_F_TREE | RTW_F_ATTR and RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR instantiations of every
// kernel family an RTW_F_ALL scene can reach) as their own translation unit: they compile beside
// rtw_wavefront.hip, and the kernels of contexts without attributes are built from exactly the instantiations
// they were (DESIGN.md §smooth shading).
#define RTW_WF_ATTRS_TU
#include "rtw_wavefront.hip"
