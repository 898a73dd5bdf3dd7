// narrowphase.hip for batches made only of boxes: the lean source with the sphere and cylinder branches of the SDF queries
// taken out by the preprocessor.  Provides launch_find_contacts_box, which launch_find_contacts hands over to when
// DssWorld.shape_box is set.  See the note at the top of narrowphase.hip.
#define DSS_BOX_ONLY 1
#include "narrowphase.hip"
