! Stand-in for the FMS header of the same name: the two macros the reference's fv_arrays.F90 expands.
#define _ALLOCATABLE allocatable
#define _NULL
