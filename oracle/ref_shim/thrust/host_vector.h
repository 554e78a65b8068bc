// Stand-in of this repository for Thrust's header of the same name (TEST INFRASTRUCTURE): the reference includes it and uses nothing of it.
#pragma once
