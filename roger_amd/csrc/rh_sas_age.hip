// rh_sas_age.hip -- the kernels of the transport bands by age, plain and per zone, and of their window means (rh_sas_age_bands.h), and their
// launches, a translation unit of its own that is linked behind every other one.  The host side (rh_sas_age_bands_*,
// rh_sas_age_window_bands_*, sas_age_bands_enqueue, sas_age_window_bands_enqueue) is rh_sas_observers.h in rh_sas.hip.
#define RH_SAS_AGE_UNIT
#include "rh_sas_age_bands.h"
