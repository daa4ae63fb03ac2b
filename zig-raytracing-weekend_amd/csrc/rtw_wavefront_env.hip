// The wavefront kernels of contexts with a registered environment (rtw_scene_set_environment: the
// RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ENV and RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR | RTW_F_ENV
// instantiations of every kernel family an RTW_F_ALL scene can reach) as their own translation unit: they compile
// beside rtw_wavefront.hip, and the kernels of contexts without an environment are built from exactly the
// instantiations they were (DESIGN.md §Environment maps).
#define RTW_WF_ENV_TU
#include "rtw_wavefront.hip"
